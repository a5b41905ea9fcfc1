# -*- coding: utf-8 -*-
"""Generates tests/golden/curve_filter.npz from the REAL reference prior/filter_curves.py (build container only):

    python tests/golden/make_golden_filter.py /path/to/reference

The reference module is imported from its path and run; only data is stored: seeded synthetic curves (ragged, concatenated),
and for each of three parameter sets the 14 integer / 12 float columns of vqvae_hip.curve_filter evaluated by the reference's
functions on the fp32 curve (ref32) and on the same curve cast to fp64 (ref64, the arbiter of tests/parity_util.py), plus what
the reference's main() did on a directory of these curves (kept files, [summary] counters, manifest records) and the
constants / CLI defaults of that main(), read with ast.

Admission (asserted): a curve enters the fixture only if its integer columns agree between ref32 and ref64 for every
parameter set and no compared quantity (pair / sample distance, bond length, angle, angle denominator, fraction) lies within
1e-4 relative of a threshold it is compared with, evaluated in fp64; otherwise the next seed is taken.  So the tests compare
integers exactly and leave no case out."""
import ast
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (1, 2, 3, 4, 17, 64, 65, 130, 350)
PER_LENGTH = 6
MARGIN = 1e-4
INT_COLUMNS = ("length", "reason", "bond_num", "bond_out", "angle_num", "angle_out", "n_self_clash_pairs", "n_seg_clash_pairs",
               "beta_total", "beta_max_run", "beta_in_sheet", "beta_strands_total", "beta_strands_sheet", "beta_strands_isolated")
FLOAT_COLUMNS = ("bond_mean", "bond_std", "bond_min", "bond_max", "bond_frac_out", "angle_mean", "angle_std", "angle_min",
                 "angle_max", "angle_frac_out", "rg", "beta_sheet_fraction")
# the three parameter sets: CLI defaults; the docstring's typical usage; all four beta rules (and max_length) active
PARAM_SETS = (
    dict(),
    dict(min_pairwise_dist=2.0, neighbor_exclude=2, min_beta_run=0, min_beta_total=0, min_length=2),
    dict(min_length=2, max_length=300, min_beta_run=4, min_beta_total=8, min_beta_sheet_fraction=0.3,
         max_isolated_beta_strands=1),
)


def load_reference(root):
    path = os.path.join(root, "prior", "filter_curves.py")
    spec = importlib.util.spec_from_file_location("ref_filter_curves", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, path


def main_constants_and_flags(path):
    """Upper-case constants assigned in main() and the add_argument flags with their defaults, as plain values."""
    tree = ast.parse(open(path).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    consts, flags = {}, {}
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) \
                and node.targets[0].id.isupper() and isinstance(node.value, (ast.Constant, ast.UnaryOp)):
            consts[node.targets[0].id] = ast.literal_eval(node.value)
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            flags[ast.literal_eval(node.args[0])] = {
                "default": ast.literal_eval(kw["default"]) if "default" in kw else None,
                "type": kw["type"].id if "type" in kw else None,
                "required": ast.literal_eval(kw["required"]) if "required" in kw else False}
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "segment_self_clash_count":
            for k in node.keywords:
                if k.arg == "num_samples":
                    consts["SEG_NUM_SAMPLES"] = ast.literal_eval(k.value)
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "beta_strand_and_sheet_stats":
            for k in node.keywords:
                if k.arg in ("threshold", "sheet_min_dist", "sheet_max_dist"):
                    consts[k.arg.upper()] = ast.literal_eval(k.value)
    return consts, flags


def full_params(flags, over):
    p = {k.lstrip("-"): v["default"] for k, v in flags.items() if not v["required"]}
    p.update(over)
    return p


# ------------------------------------------------------------------------------------------------ curves
def walk(seed, L, ss=True):
    """Protein-like walk: step 3.8 +- 0.15 A, direction persistence 0.5 / 0.7 / 0.85, optional pull towards the origin
    (compact, clashing curves), SS labels in blocks of 4."""
    g = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v)
    pers = (0.5, 0.7, 0.85)[seed % 3]
    pull = (0.0, 0.0, 0.35, 0.7)[(seed // 3) % 4]
    pos, d, pts = np.zeros(3), unit(g.standard_normal(3)), []
    for _ in range(L):
        pts.append(pos.copy())
        d = unit(pers * d + (1.0 - pers) * unit(g.standard_normal(3)) - pull * pos / (np.linalg.norm(pos) + 3.8))
        pos = pos + d * (3.8 + 0.15 * g.standard_normal())
    xyz = np.asarray(pts, np.float32)
    if not ss:
        return xyz
    lab = np.repeat(g.integers(0, 3, (L + 3) // 4), 4)[:L]
    return np.concatenate([xyz, np.eye(3, dtype=np.float32)[lab]], 1)


def zigzag(L, bond=3.8):
    """A clean planar zigzag (angle ~ 110 degrees, nothing near a threshold) with a slow drift out of the plane."""
    k = np.arange(L)
    half = np.deg2rad(110.0) / 2
    xyz = np.stack([k * bond * np.sin(half), (k % 2) * bond * np.cos(half), 0.37 * k], 1)
    return xyz.astype(np.float32)


def with_ss(xyz, lab):
    return np.concatenate([xyz, np.eye(3, dtype=np.float32)[np.asarray(lab)]], 1).astype(np.float32)


def handmade():
    out = []
    a = zigzag(40); a[20:] += np.float32([4.9, 0, 0]); out.append(("bond_8A", with_ss(a, [2] * 40)))
    a = zigzag(40); a[20:] -= np.float32([1.9, 0, 0]); out.append(("bond_1p5A", with_ss(a, [0] * 40)))
    a = zigzag(40); a[11] = a[10]; out.append(("coincident", with_ss(a, [2] * 40)))
    out.append(("no_ss", zigzag(48)))
    # hairpin: two antiparallel beta strands 4.8 A apart (sheet partners), a loop, then an isolated strand far away
    s1 = zigzag(10)
    s2 = zigzag(10)[::-1] + np.float32([0, 0, 4.8 + 3.7])
    s2[:, 2] -= 2 * 0.37 * np.arange(10)[::-1]
    loop = np.float32([[33.5, 1.0, 5.2], [35.5, 2.0, 7.5]])
    tail = zigzag(12)[:, [1, 0, 2]] + np.float32([-3.0, -6.0, 10.0])
    xyz = np.concatenate([s1, loop, s2, tail])
    lab = [1] * 10 + [2] * 2 + [1] * 10 + [2] * 3 + [1] * 6 + [2] * 3
    out.append(("hairpin", with_ss(xyz, lab)))
    # sharp turn: one angle of about 6 degrees
    a = zigzag(40); a[21:] = a[21:] - a[21] + a[19] + np.float32([0.35, 0.1, 0.2]); out.append(("sharp", with_ss(a, [0] * 40)))
    return out


# ------------------------------------------------------------------------------------------------ reference evaluation
class Evaluator:
    def __init__(self, ref, consts):
        self.ref, self.c = ref, consts
        self.cache = {}

    def base(self, key, curve):
        """Parameter-independent statistics of one curve at one precision (cached: the segment count is slow)."""
        if key not in self.cache:
            R, c = self.ref, self.c
            xyz = curve[:, :3]
            self.cache[key] = dict(
                bl=R.bond_length_stats(xyz, good_min=c["BOND_GOOD_MIN"], good_max=c["BOND_GOOD_MAX"]),
                ba=R.bond_angle_stats(xyz, good_min_deg=c["ANGLE_GOOD_MIN"], good_max_deg=c["ANGLE_GOOD_MAX"]),
                rg=R.radius_of_gyration(xyz),
                seg=R.segment_self_clash_count(xyz, min_seg_dist=c["SEG_MIN_DIST"],
                                               neighbor_exclude_segments=c["SEG_NEIGHBOR_EXCLUDE"],
                                               num_samples=c["SEG_NUM_SAMPLES"]))
        return self.cache[key]

    def columns(self, key, curve, p):
        """All 14 + 12 columns: the reference's functions, chained in the order of its main()."""
        R, c = self.ref, self.c
        b = self.base(key, curve)
        bl, ba, L, xyz = b["bl"], b["ba"], curve.shape[0], curve[:, :3]
        pt = R.self_collision_stats(xyz, min_pairwise_dist=float(p["min_pairwise_dist"]),
                                    neighbor_exclude=int(p["neighbor_exclude"]))
        bt = bm = 0
        st = dict(beta_in_sheet=0, beta_sheet_fraction=0.0, n_strands_total=0, n_sheet_strands=0, n_isolated_strands=0)
        ss_rej = False
        if curve.shape[1] >= 6:
            ss = curve[:, 3:6]
            bt, bm = R.beta_stats(ss, beta_channel=int(p["beta_channel"]))
            st = R.beta_strand_and_sheet_stats(coords=xyz, ss_one_hot=ss, beta_channel=int(p["beta_channel"]),
                                               threshold=c["THRESHOLD"], neighbor_exclude=int(p["neighbor_exclude"]),
                                               min_strand_len=int(p["min_strand_len"]), sheet_min_dist=c["SHEET_MIN_DIST"],
                                               sheet_max_dist=c["SHEET_MAX_DIST"])
            ss_rej |= p["min_beta_total"] > 0 and 0 < bt < p["min_beta_total"]
            ss_rej |= p["min_beta_run"] > 0 and bt > 0 and bm < p["min_beta_run"]
            ss_rej |= p["min_beta_sheet_fraction"] > 0.0 and bt > 0 and st["beta_sheet_fraction"] < p["min_beta_sheet_fraction"]
            ss_rej |= p["max_isolated_beta_strands"] >= 0 and st["n_isolated_strands"] > p["max_isolated_beta_strands"]
        if L < p["min_length"]:
            reason = 1
        elif p["max_length"] > 0 and L > p["max_length"]:
            reason = 2
        elif bl["num"] > 0 and (bl["min"] < c["BOND_MIN_ALLOWED"] or bl["max"] > c["BOND_MAX_ALLOWED"]
                                or bl["frac_out"] > c["BOND_FRAC_OUT_MAX"]):
            reason = 3
        elif ba["num"] > 0 and (ba["min"] < c["ANGLE_MIN_ALLOWED"] or ba["max"] > c["ANGLE_MAX_ALLOWED"]
                                or ba["frac_out"] > c["ANGLE_FRAC_OUT_MAX"]):
            reason = 4
        elif pt > 0:
            reason = 5
        elif b["seg"] > 0:
            reason = 6
        else:
            reason = 7 if ss_rej else 0
        ints = [L, reason, bl["num"], round(bl["frac_out"] * bl["num"]), ba["num"], round(ba["frac_out"] * ba["num"]), pt,
                b["seg"], bt, bm, st["beta_in_sheet"], st["n_strands_total"], st["n_sheet_strands"], st["n_isolated_strands"]]
        floats = [bl["mean"], bl["std"], bl["min"], bl["max"], bl["frac_out"], ba["mean"], ba["std"], ba["min"], ba["max"],
                  ba["frac_out"], b["rg"], st["beta_sheet_fraction"]]
        return np.asarray(ints, np.int32), np.asarray(floats, np.float64)


def near(vals, thr):
    vals = np.asarray(vals, np.float64)
    return bool(vals.size) and bool(np.any(np.abs(vals - thr) <= MARGIN * abs(thr)))


def margins_ok(curve, consts, psets):
    """fp64: no compared quantity within MARGIN (relative) of a threshold it is compared with."""
    x = curve[:, :3].astype(np.float64)
    L = x.shape[0]
    c = consts
    if L >= 2:
        d = np.linalg.norm(x[1:] - x[:-1], axis=-1)
        if any(near(d, c[k]) for k in ("BOND_MIN_ALLOWED", "BOND_MAX_ALLOWED", "BOND_GOOD_MIN", "BOND_GOOD_MAX")):
            return False
        if near([np.mean((d < c["BOND_GOOD_MIN"]) | (d > c["BOND_GOOD_MAX"]))], c["BOND_FRAC_OUT_MAX"]):
            return False
    if L >= 3:
        v1, v2 = x[:-2] - x[1:-1], x[2:] - x[1:-1]
        den = np.linalg.norm(v1, axis=-1) * np.linalg.norm(v2, axis=-1)
        if near(den, 1e-6):
            return False
        ok = den > 1e-6
        ang = np.degrees(np.arccos(np.clip((v1[ok] * v2[ok]).sum(-1) / den[ok], -1.0, 1.0)))
        if any(near(ang, c[k]) for k in ("ANGLE_MIN_ALLOWED", "ANGLE_MAX_ALLOWED", "ANGLE_GOOD_MIN", "ANGLE_GOOD_MAX")):
            return False
        if ang.size and near([np.mean((ang < c["ANGLE_GOOD_MIN"]) | (ang > c["ANGLE_GOOD_MAX"]))], c["ANGLE_FRAC_OUT_MAX"]):
            return False
    ne = min(int(p["neighbor_exclude"]) for p in psets)
    i, j = np.triu_indices(L, ne + 1)
    dist = np.linalg.norm(x[i] - x[j], axis=-1)
    for thr in {float(p["min_pairwise_dist"]) for p in psets} | {c["SHEET_MIN_DIST"], c["SHEET_MAX_DIST"]}:
        if near(dist, thr):
            return False
    if L >= 3:
        t = np.linspace(0.0, 1.0, c["SEG_NUM_SAMPLES"])
        pts = x[:-1, None, :] + (x[1:] - x[:-1])[:, None, :] * t[None, :, None]          # [nseg, S, 3]
        i, j = np.triu_indices(L - 1, 1 + c["SEG_NEIGHBOR_EXCLUDE"])
        for s in range(0, i.size, 20000):
            dd = np.linalg.norm(pts[i[s:s + 20000], :, None, :] - pts[j[s:s + 20000], None, :, :], axis=-1)
            if near(dd, c["SEG_MIN_DIST"]):
                return False
    return True


def evaluate(ev, key, curve, consts, psets):
    """-> (ints [P,14], f32 [P,12], f64 [P,12]) or None when the curve is not admitted."""
    if not margins_ok(curve, consts, psets):
        return None
    I, F32, F64 = [], [], []
    for p in psets:
        i32, f32 = ev.columns((key, 32), curve.astype(np.float32), p)
        i64, f64 = ev.columns((key, 64), curve.astype(np.float64), p)
        if not np.array_equal(i32, i64):
            return None
        if p["min_beta_sheet_fraction"] > 0 and i64[8] > 0 and near([f64[11]], p["min_beta_sheet_fraction"]):
            return None
        I.append(i32); F32.append(f32); F64.append(f64)
    return np.stack(I), np.stack(F32), np.stack(F64)


# ------------------------------------------------------------------------------------------------ the reference's main()
def file_name(k):
    return f"sample_prior_{k:04d}{'x' if k % 11 == 7 else ''}_recon.npy"       # every 11th name carries no parsable index


def samples_manifest(n):
    lines = []
    for k in range(n):
        if k % 3 == 0:
            lines.append({"i": k, "indices_path": f"codes/sample_prior_{k:04d}.npy", "length": 64 + k, "tag": f"t{k}"})
        elif k % 3 == 1:
            lines.append({"indices_path": f"codes/sample_prior_{k:04d}.npy", "temperature": 0.5 + 0.01 * k})
    lines.append({"indices_path": "codes/no_index_here.npy"})
    return lines


def run_main(ref, curves, over, manifest_lines):
    with tempfile.TemporaryDirectory() as tmp:
        rdir, odir = os.path.join(tmp, "recon"), os.path.join(tmp, "out")
        os.makedirs(rdir)
        for k, cv in enumerate(curves):
            np.save(os.path.join(rdir, file_name(k)), cv)
        mpath, fpath = os.path.join(tmp, "samples.jsonl"), os.path.join(tmp, "filtered.jsonl")
        with open(mpath, "w") as f:
            f.write("\n".join(json.dumps(r) for r in manifest_lines) + "\n\nnot json\n")
        argv = ["filter_curves.py", "--recon_dir", rdir, "--out_dir", odir, "--samples_manifest", mpath,
                "--filtered_manifest_out", fpath]
        for k, v in over.items():
            argv += [f"--{k}", str(v)]
        buf, old = io.StringIO(), sys.argv
        sys.argv = argv
        try:
            with contextlib.redirect_stdout(buf):
                ref.main()
        finally:
            sys.argv = old
        summary = [int(line.rsplit(":", 1)[1]) for line in buf.getvalue().splitlines() if line.startswith("[summary]")]
        kept = sorted(os.listdir(odir))
        recs = [json.loads(line) for line in open(fpath)]
        for r in recs:
            r["recon_path"] = os.path.basename(r["recon_path"])
        return kept, summary, recs


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ref, path = load_reference(root)
    consts, flags = main_constants_and_flags(path)
    psets = [full_params(flags, o) for o in PARAM_SETS]
    ev = Evaluator(ref, consts)
    curves, names, seeds, rows = [], [], [], []
    t0 = time.time()
    seed = 1000
    for L in LENGTHS:
        got = 0
        while got < PER_LENGTH:
            seed += 1
            cv = walk(seed, L)
            r = evaluate(ev, ("walk", seed), cv, consts, psets)
            if r is None:
                print(f"[skip] seed {seed} L {L}: not admitted")
                continue
            curves.append(cv); names.append(f"walk_L{L}_s{seed}"); seeds.append(seed); rows.append(r)
            got += 1
    for name, cv in handmade():
        r = evaluate(ev, ("hand", name), cv, consts, psets)
        assert r is not None, f"hand-made curve {name} is not admitted"
        curves.append(cv); names.append(name); seeds.append(-1); rows.append(r)
    # one curve given as SS logits with an exact tie: its argmax one-hot is what the reference sees
    g = np.random.default_rng(77)
    base = walk(2001, 64)
    logits = g.standard_normal((64, 3)).astype(np.float32)
    logits[5] = [0.75, 0.75, -1.0]                     # exact tie: first maximum (channel 0) wins
    logits[6] = [-0.5, 1.25, 1.25]                     # exact tie: channel 1 wins over channel 2
    logits[7] = [2.0, 2.0, 2.0]
    logits_curve = np.concatenate([base[:, :3], logits], 1)
    onehot = np.concatenate([base[:, :3], np.eye(3, dtype=np.float32)[np.argmax(logits, 1)]], 1)
    r = evaluate(ev, ("hand", "logits"), onehot, consts, psets)
    assert r is not None, "logits curve is not admitted"
    logits_index = len(curves)
    curves.append(onehot); names.append("logits_tie"); seeds.append(2001); rows.append(r)
    per_curve = (time.time() - t0)
    ints = np.stack([r[0] for r in rows], 1)           # [P, N, 14]
    f32 = np.stack([r[1] for r in rows], 1)
    f64 = np.stack([r[2] for r in rows], 1)
    reasons = set(ints[:, :, 1].reshape(-1).tolist())
    assert reasons == set(range(8)), f"reason codes covered: {sorted(reasons)}"
    print("reason histogram per set:", [np.bincount(ints[p, :, 1], minlength=8).tolist() for p in range(len(psets))])
    print("max ordered point-collision count", ints[:, :, 6].max(), "max segment clash count", ints[:, :, 7].max(),
          "min angle", f32[0, :, 7][ints[0, :, 4] > 0].min(), "sheet strands", ints[:, :, 12].max(),
          "isolated strands", ints[:, :, 13].max())

    # the reference's main() on a directory of these curves
    manifest_lines = samples_manifest(len(curves))
    out = {}
    for p, over in enumerate(PARAM_SETS):
        kept, summary, recs = run_main(ref, curves, over, manifest_lines)
        kept_idx = [k for k in range(len(curves)) if file_name(k) in kept]
        assert kept_idx == [k for k in range(len(curves)) if ints[p, k, 1] == 0], "main() and the column chain disagree"
        hist = np.bincount(ints[p, :, 1], minlength=8)
        assert summary == [len(curves), int(hist[0])] + hist[1:].tolist(), (summary, hist)
        assert len(recs) == len(kept_idx)
        out[f"main{p}_kept"] = np.asarray(kept_idx, np.int32)
        out[f"main{p}_summary"] = np.asarray(summary, np.int32)
        out[f"main{p}_records"] = np.asarray([json.dumps(r) for r in recs])
    # a capped run (--max_curves 5) of the second set: the reference stops reading files at the fifth kept curve
    kept, summary, recs = run_main(ref, curves, dict(PARAM_SETS[1], max_curves=5), manifest_lines)
    out["main1_cap5_kept"] = np.asarray([k for k in range(len(curves)) if file_name(k) in kept], np.int32)
    out["main1_cap5_summary"] = np.asarray(summary, np.int32)

    lens = np.asarray([c.shape[0] for c in curves], np.int32)
    chans = np.asarray([c.shape[1] for c in curves], np.int32)
    flat = np.zeros((int(lens.sum()), 6), np.float32)
    o = 0
    for c in curves:
        flat[o:o + c.shape[0], :c.shape[1]] = c
        o += c.shape[0]
    file_names = [file_name(k) for k in range(len(curves))]
    name_index = [ref.extract_index_from_name(n) for n in file_names]
    np.savez_compressed(
        os.path.join(HERE, "curve_filter.npz"), curves=flat, lengths=lens, channels=chans, names=np.asarray(names),
        seeds=np.asarray(seeds, np.int32), logits_index=np.int32(logits_index), logits_curve=logits_curve,
        ints=ints, f32=f32.astype(np.float64), f64=f64, int_columns=np.asarray(INT_COLUMNS), float_columns=np.asarray(FLOAT_COLUMNS),
        param_sets=np.asarray([json.dumps(p) for p in psets]), param_overrides=np.asarray([json.dumps(p) for p in PARAM_SETS]),
        main_constants=np.asarray(json.dumps(consts)), cli_flags=np.asarray(json.dumps(flags)),
        file_names=np.asarray(file_names), name_index=np.asarray([-1 if v is None else v for v in name_index], np.int32),
        samples_manifest=np.asarray([json.dumps(r) for r in manifest_lines]),
        ref_seconds_total=np.float64(per_curve), **out)
    print(f"wrote curve_filter.npz: {len(curves)} curves, {flat.shape[0]} points, reference evaluation {per_curve:.1f} s "
          f"on 1 core ({os.cpu_count()} present), file {os.path.getsize(os.path.join(HERE, 'curve_filter.npz')) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
