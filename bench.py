# -*- coding: utf-8 -*-
"""
bench.py -- training throughput of the VQ-VAE hot path on N MI355X (one process per GPU).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus N ...          (no RANK in the environment: starts N ranks itself as child processes, below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

Default workload = config C2 (stage2_vq.yaml model with num_quantizers=1, codebook K=512, D=64,
N=64 latent tokens), the configuration BASELINE.json's metric is quoted on.  A "step" = one full training step on a
per-rank batch of 256 synthetic curve tensors [256, 64, 6] already resident in HBM: forward (dropout 0.1 active) +
24-term loss + backward + RCCL all-reduce (N>1) + global-norm clip + AdamW + EMA codebook refresh, all fp32.
Prints ONE JSON line (rank 0) with the whole-job samples/s and ms_per_step.  With --full it also measures the roofline of
the dominant kernel (the GEMM instantiation with the largest summed time, measured live with HIP events on the launch stream
over two extra eager steps) and a CPU baseline (the oracle timed on the host cores; it is imported only inside that leg);
a plain run does neither and reports both as null.
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (see dump_step_outputs).

Other BASELINE shapes, for profiling (not the judged bench line):   --workload c4 | c5 | stage2
The real-data path end to end (ragged lengths -> DataLoader -> pad_collate -> bucketed step):   --workload realdata
The quantizer alone at SURVEY 8d's image-derived shapes (one JSON line per shape):   --vq-only
(--full adds the quantizer's roofline and CPU baseline there, and the fixed-shape comparison to realdata)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "pytorch-vae_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import yaml  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3          # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 2500.0         # same guide, "Peak BF16/FP16 MFMA": ~2.5 PF dense
X3_PRODUCTS = 6                        # bf16 MFMA products executed per fp32 product by the split-operand kernels (gemm_dma.inc)
BENCH_EPOCH = 100                      # loss weights = stage2 schedules evaluated at this epoch (all terms on)
# matmul FLOPs fwd+bwd per sample (reference graph, FlopCounterMode)
WORKLOADS = {
    "c2": dict(desc="C2: stage2_vq.yaml model with num_quantizers=1 K=512 D=64 N=64", batch=256, seq=64, gflop=16.846,
               over=dict(num_quantizers=1, codebook_size=512, code_dim=64, latent_tokens=64)),
    "c4": dict(desc="C4 stage-2 shape: C2 model at L=256, B=1024 (96 GiB of activations)", batch=1024, seq=256, gflop=61.849,
               over=dict(num_quantizers=1, codebook_size=512, code_dim=64, latent_tokens=64)),
    "c5": dict(desc="C5 per-rank shape: K=8192 D=256 Q=1, L=256, B=64", batch=64, seq=256, gflop=62.453,
               over=dict(num_quantizers=1, codebook_size=8192, code_dim=256, latent_tokens=64)),
    "stage2": dict(desc="stage2_vq.yaml verbatim (RVQ 4x1024, D=512, N=64), L=256, B=256", batch=256, seq=256, gflop=63.359,
                   over=dict()),
}
VQ_SHAPES = [(65536, 512, 64), (262144, 8192, 256)]     # R = B*16*16 rows of the upstream image VQ-VAE
DUMP_SAMPLE = 1 << 21                                   # positions sampled from the weights / gradients: 8 MB of float32 each


def setup(workload):
    from experiment import interpolate_schedule
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "stage2_vq.yaml")))
    mp = dict(cfg["model_params"])
    mp.update(WORKLOADS[workload]["over"])
    mp.update(reinit_dead_codes=False, print_init=False)
    ep = cfg["exp_params"]
    sched = interpolate_schedule(ep["schedules"], BENCH_EPOCH)
    keys = ["ss_weight", "bond_length_weight", "bond_angle_weight", "xyz_tv_lambda", "dir_weight", "dih_weight",
            "rmsd_weight", "pdm_weight", "win_kabsch_weight", "kappa_weight", "tau_weight", "lr_pdm_weight",
            "pdm_window", "win_kabsch_size", "win_kabsch_stride", "lr_min_sep", "lr_stride", "lr_max_offsets"]
    weights = {k: float(sched.get(k, ep.get(k, 0.0))) for k in keys}
    hp = dict(lr=float(sched.get("LR", ep["LR"])), wd=float(ep["weight_decay"]),
              clip=float(cfg["trainer_params"]["gradient_clip_val"]), beta=float(sched.get("beta", mp["beta"])),
              seed=int(ep["manual_seed"]))
    return mp, weights, hp


def c2_setup():
    return setup("c2")


def synthetic_batch(B, L, seed, device):
    from dataset import synthetic_curve_batch
    x, mask = synthetic_curve_batch(B, L, seed, ragged=False)
    return x.to(device), mask.to(device)


def cpu_baseline(mp, weights, hp, B_cpu=256, L=64, steps=2):
    """The oracle (kind 'port': our CPU restatement, verified against the reference by the golden vectors) timed on the
    host cores for the same model / step at the metric's own batch (same config, 1 warm-up + 2 timed steps,
    ~9 s each on 16 cores).  The only place bench.py touches oracle/."""
    from dataset import synthetic_curve_batch
    from oracle import vqvae_oracle as O
    ncores = min(16, os.cpu_count() or 1)
    torch.set_num_threads(ncores)
    torch.manual_seed(hp["seed"])
    cfg = O.make_cfg(**mp)
    sd = O.attach_grads(O.random_state(cfg, hp["seed"]), cfg)
    orc = O.OracleVQVAE(sd, drop_scale=1.0, **mp)
    orc.beta = hp["beta"]
    orc.training_steps = 1
    opt = torch.optim.AdamW(orc.params(), lr=hp["lr"], weight_decay=hp["wd"])
    x, mask = synthetic_curve_batch(B_cpu, L, 7, ragged=False)
    orc.train_step(x, mask, opt, hp["clip"], weights)          # warm-up
    t0 = time.time()
    for _ in range(steps):
        orc.train_step(x, mask, opt, hp["clip"], weights)
    dt = (time.time() - t0) / steps
    return {"value": round(B_cpu / dt, 3), "unit": "images/s", "cores": ncores, "kind": "port",
            "sample": f"oracle train step (dropout 0.1, AdamW+clip), B={B_cpu} L={L}, {steps} timed steps after 1 warm-up"}


def dump_step_outputs(model, eng, out_dir):
    """--dump-outputs: what the last training step handed its caller, as float32 .npy files -- `metrics` (the vector
    train_step returns, engine.METRIC_KEYS order), `params` / `grads` (the updated weights and the step's gradients,
    concatenated in named_parameters order; above DUMP_SAMPLE elements a fixed seeded sample of positions, the same in
    every run of the same model) and the quantizer's buffers (codebook, EMA statistics) whole."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    named = list(model.named_parameters())
    w = torch.cat([p.detach().reshape(-1) for _, p in named])
    g = torch.cat([eng.G[n].reshape(-1) for n, _ in named])
    if w.numel() > DUMP_SAMPLE:
        pos = np.unique(np.random.default_rng(1234).integers(0, w.numel(), DUMP_SAMPLE))
        pos = torch.from_numpy(pos).to(w.device)
        w, g = w[pos], g[pos]
    arrays = {"metrics": eng.metrics, "params": w, "grads": g}
    arrays.update({n: b for n, b in model.named_buffers() if n.startswith("quantizer.") and b.is_floating_point()})
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())


def pmc_traffic(kernel_name):
    """HBM bytes per launch of `kernel_name` from the newest committed rocprofv3 --pmc summary under profiles/ (collected
    in separate passes and corrected as MI355X_MICROARCH.md prescribes; see profiles/README.md), or None."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_c2_pmc_traffic.json")), reverse=True):
        try:
            pm = json.load(open(path))
        except Exception:
            continue
        for pk, d in pm.items():
            if kernel_name in pk and isinstance(d, dict) and "hbm_bytes_per_launch_corrected" in d:
                return d["hbm_bytes_per_launch_corrected"], os.path.basename(path)
    return None, None


def bench_vq_only(args, dev):
    """VectorQuantizerEMA.forward alone (models/vq_vae.py:170-223: distances + argmin + gather + EMA update + usage stats) at the
    image-derived shapes; roofline = the nearest-neighbour kernel's 2*R*K*D against the fp32 MFMA peak."""
    from models.vq_vae import VQVAE
    from vqvae_hip import lib as L
    for R, K, D in VQ_SHAPES:
        Bq, M = R // 256, 256
        m = VQVAE(hidden_dim=64, num_heads=4, tokenizer_heads=4, codebook_size=K, code_dim=D, latent_tokens=M, use_vq=True,
                  reinit_dead_codes=False, print_init=False).to(dev).train()
        eng = m._engine()
        q = m.quantizer
        g = torch.Generator().manual_seed(R + K)
        z = torch.randn(R, D, generator=g).to(dev)
        emb = (torch.randn(K, D, generator=g) / D ** 0.5).to(dev)
        q.embedding.copy_(emb); q.ema_embedding.copy_(emb); q.ema_cluster_size.fill_(1.0)
        eng.train, eng.defer_ema = True, False
        eng.use_arena(("vq", Bq, M))

        def step():
            eng.quantize(z, Bq, True)
        for _ in range(max(args.warmup, 2)):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        out = {"metric": "VectorQuantizerEMA.forward rows/sec (nearest + gather + EMA update + usage stats)",
               "value": round(R * args.steps / el, 1), "unit": "rows/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(el / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32", "gemm_arithmetic": ("bf16x3 exact split (6 products, fp32 accumulate)" if args.gemm == "x3"
                                                   else "native fp32 MFMA"),
               "data": "synthetic",
               "config": {"workload": f"vq-only R={R} K={K} D={D} (SURVEY.md 8d image-derived shape), fresh centroid-initialised table"},
               "roofline": None, "cpu_baseline": None}
        if not args.full:
            print(json.dumps(out), flush=True)
            continue
        n, t, f = L.vq_profile(lambda: [step() for _ in range(3)])
        # which score kernel ran (csrc/vq.hip dispatch): D = 64 / 128 / 256 -> the split-operand kernel on the bf16 pipes
        # (6 bf16 MFMA products per fp32 product) unless vqh_vq_set_flags bit 1 asks for the fp32 MFMA form
        vq_x3 = D in (64, 128, 256) and args.gemm == "x3"
        mult, peak = (X3_PRODUCTS, BF16_MFMA_PEAK_TFLOPS) if vq_x3 else (1, FP32_MFMA_PEAK_TFLOPS)
        # form 3 = the plane-tensor kernel (D = 128 / 256, workspace permitting; its launch interval also holds the two operand
        # split kernels, which belong to the form's cost), 2 = Z rows as register-resident planes
        form = int(L.lib().vqh_vq_nearest_form(R, K, D, eng.ws.numel()))
        kname = {3: "vq_nearest_p3_kernel (+ 2 x p3_split_tiled_kernel)", 2: "vq_nearest_x3_kernel<%d>" % (D // 16),
                 1: "vq_nearest_lds_kernel<%d>" % (D // 8), 0: "vq_nearest_kernel"}[form]
        vq_roof = {"bound": "mfma", "kernel": kname,
                   "achieved": round(mult * f / t / 1e12, 2), "peak": peak, "unit": "TFLOP/s",
                   "frac": round(mult * f / t / 1e12 / peak, 4),
                   "arithmetic": ("bf16 MFMA on exact 3-way splits, 6 products per fp32 product (executed flops = 6 x 2RKD)" if vq_x3
                                  else "fp32 MFMA"),
                   "fp32_equivalent": {"achieved": round(f / t / 1e12, 2), "unit": "TFLOP/s", "what": "algorithmic 2*R*K*D / kernel time"},
                   "traffic": None, "avg_launch_us": round(t / n * 1e6, 2), "gflop_per_launch": round(f / n / 1e9, 3)}
        cpu = None
        if not args.no_cpu_baseline:
            from oracle import vqvae_oracle as O
            ncores = min(16, os.cpu_count() or 1)
            torch.set_num_threads(ncores)
            Rc = min(R, 16384 if K > 4096 else 65536)            # bounded sample: the oracle materialises Rc x K floats twice
            cfgq = dict(codebook_size=K, code_dim=D, num_quantizers=1, use_vq=True)
            sd = {k: torch.zeros(s) for k, s in O.buffer_shapes(O.make_cfg(**cfgq)).items() if k.startswith("quantizer.")}
            sd["quantizer.embedding"] = emb.cpu().clone()
            sd["quantizer.ema_embedding"] = emb.cpu().clone()
            sd["quantizer.ema_cluster_size"] = torch.ones(K)
            orc = O.OracleVQVAE(sd, **cfgq)
            orc.training = True
            zc = z[:Rc].cpu().view(Rc // 256, 256, D)
            orc.quantize(zc, do_ema_update=True)
            tc = time.time()
            reps = 3
            for _ in range(reps):
                orc.quantize(zc, do_ema_update=True)
            dtc = (time.time() - tc) / reps
            cpu = {"value": round(Rc / dtc, 1), "unit": "rows/s", "cores": ncores, "kind": "port",
                   "sample": f"oracle VectorQuantizerEMA.forward (train mode), R={Rc} of {R} rows, {reps} timed calls"}
        out.update(roofline=vq_roof, cpu_baseline=cpu)
        print(json.dumps(out), flush=True)


def bench_realdata(args, dev):
    """The real-data path end to end: stage2_vq.yaml VERBATIM (RVQ 4x1024, D=512, train_batch_size 128,
    max_seq_len 350) driven the way run.py drives it -- SyntheticCurveDataset curves with lengths U[175, 350] -> DataLoader
    workers -> pad_collate (each batch padded to its own L_max, reference dataset.py:30-49) -> pinned host batch ->
    VQVAEExperiment.training_step -> length-bucketed fused step (hipGraph per bucket).  Reported next to the same engine
    stepping on ONE device-resident batch of the dominant bucket shape (no loader, no H2D, no shape changes): the gap
    between the two is what the host side costs."""
    import types
    from experiment import VQVAEExperiment
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "stage2_vq.yaml")))
    mp, ep, dp = dict(cfg["model_params"]), dict(cfg["exp_params"]), dict(cfg["data_params"])
    mp.update(print_init=False)
    B = int(args.batch or dp.get("train_batch_size", 128))
    warm, steps = max(args.warmup, 6), args.steps
    dp.update(train_batch_size=B, num_workers=4, pin_memory=True,
              synthetic={"n": B * (warm + steps), "n_val": B, "max_len": int(mp.get("max_seq_len", 350)),
                         "min_len": int(mp.get("max_seq_len", 350)) // 2, "seed": 5})
    ep.update(print_every=0)
    torch.manual_seed(int(ep["manual_seed"]))
    exp = VQVAEExperiment(mp, ep, dp)
    exp.trainer = types.SimpleNamespace(max_epochs=1, gradient_clip_val=float(cfg["trainer_params"]["gradient_clip_val"]),
                                        ckpt_path=None)
    exp.model = exp.model.to(dev).train()
    exp.setup("fit")
    exp.configure_optimizers()
    exp.current_epoch = BENCH_EPOCH                      # schedules at the epoch the other workloads use (all terms on)
    exp.on_train_epoch_start()
    eng = exp.model._engine()
    shapes, modes, t0 = [], [], None
    for i, batch in enumerate(exp.train_dataloader()):
        if i == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        exp.training_step(batch, i)
        shapes.append((int(batch[0].shape[1]), eng.arena.key[1]))
        modes.append(eng.last_step_mode)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    n_timed = len(shapes) - warm
    loss_end = float(eng.metrics[0])
    if args.dump_outputs:
        dump_step_outputs(exp.model, eng, args.dump_outputs)
    fixed = None
    if args.full:
        # the same engine on one resident batch of the dominant bucket shape
        Lb = max(set(b for _, b in shapes[warm:]), key=[b for _, b in shapes[warm:]].count)
        from dataset import synthetic_curve_batch
        x, mask = (t.to(dev) for t in synthetic_curve_batch(B, Lb, 4321, ragged=True, min_len=Lb // 2))
        w, lr, wd, clip = exp.loss_weights(), exp.lr_policy.current()[0], exp.weight_decay, exp.trainer.gradient_clip_val
        for _ in range(3):
            eng.train_step(x, mask, w, lr, wd, clip)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n_timed):
            eng.train_step(x, mask, w, lr, wd, clip)
        torch.cuda.synchronize()
        el_fixed = time.perf_counter() - t1
        fixed = {"value": round(B * n_timed / el_fixed, 2), "ms_per_step": round(el_fixed / n_timed * 1e3, 3),
                 "what": f"same engine, one device-resident ragged batch [B={B}, L={Lb}], graph replay"}
    out = {"metric": "train images/sec, real-data path (ragged curves -> DataLoader -> pad_collate -> bucketed fused step)",
           "value": round(B * n_timed / el, 2), "unit": "images/s", "n_gpus": 1, "steps": n_timed, "warmup": warm,
           "ms_per_step": round(el / n_timed * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"stage2_vq.yaml verbatim, B={B}, lengths U[{dp['synthetic']['min_len']},{dp['synthetic']['max_len']}], "
                                  f"4 loader workers, pinned batches, length buckets of {eng.len_bucket}",
                      "raw_L_max_seen": sorted(set(a for a, _ in shapes)), "buckets_seen": sorted(set(b for _, b in shapes)),
                      "arenas": len(eng.arenas) - 1,
                      "step_modes_timed": {mo: modes[warm:].count(mo) for mo in sorted(set(modes[warm:]))}},
           "fixed_shape": fixed, "realdata_over_fixed": round(el_fixed / el, 4) if fixed else None, "loss": round(loss_end, 5)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["realdata"], default="c2")
    ap.add_argument("--batch", type=int, default=0, help="per-rank batch (weak scaling); 0 = the workload's own")
    ap.add_argument("--seq", type=int, default=0)
    ap.add_argument("--vq-only", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--gemm", choices=["x3", "native"], default="x3",
                    help="large GEMM tiles: x3 = bf16 matrix pipes fed by an exact 3-way split of the fp32 operands (default); "
                         "native = v_mfma_f32_32x32x2_f32")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the dominant kernel's roofline (two extra eager "
                         "steps), the CPU baseline, the fixed-shape comparison of --workload realdata")
    ap.add_argument("--no-kernel-profile", action="store_true", help="with --full: skip the two eager HIP-event-timed steps (rocprofv3 runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed as DIR/<name>.npy (float32, under 64 MB)")
    args = ap.parse_args()
    if args.dump_outputs and args.vq_only:
        ap.error("--dump-outputs: the --vq-only bench writes no outputs")

    # --gpus N without a launcher: start the N ranks ourselves, as CHILD processes, before anything touches the GPU
    # (a process that has initialised HIP is never re-exec'ed); rank 0 of the children prints the JSON line.
    from vqvae_hip import launch
    if args.gpus > 1 and not launch.under_launcher():
        raise SystemExit(launch.spawn_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:]))
    rank = int(os.environ.get("RANK", 0))
    local = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch {args.gpus} ranks "
                         f"(python bench.py --gpus {args.gpus} does it itself) or pass --gpus {world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs MI355X GPUs (the HIP path has no CPU fallback)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if args.vq_only:
        if args.gemm == "native":
            from vqvae_hip import lib as L
            L.lib().vqh_vq_set_flags(L.lib().vqh_vq_set_flags(0) | 2)
        return bench_vq_only(args, dev)
    if args.workload == "realdata":
        return bench_realdata(args, dev)
    dist = torch.distributed
    selftest = os.environ.get("VQH_DP_SELFTEST") == "1"      # one-rank RCCL group: exercises the N>1 code path on one GPU
    if world > 1 or selftest:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)

    from models import vae_models
    from vqvae_hip import lib as L
    if args.gemm == "native":
        L.lib().vqh_gemm_set_flags(L.lib().vqh_gemm_set_flags(1) | L.GEMM_FLAG_NATIVE_F32)
    wl = WORKLOADS[args.workload]
    mp, weights, hp = setup(args.workload)
    torch.manual_seed(hp["seed"])                        # same initial weights on every rank (DDP semantics)
    model = vae_models["VQVAE"](**mp).to(dev).train()
    model.beta = hp["beta"]
    eng = model._engine()
    eng.rng[0] = hp["seed"] + 1000 * rank                # decorrelated dropout per rank
    B, Lq = args.batch or wl["batch"], args.seq or wl["seq"]
    x, mask = synthetic_batch(B, Lq, 1000 + rank, dev)

    def step():
        return eng.train_step(x, mask, weights, hp["lr"], hp["wd"], hp["clip"], use_graph=not args.no_graph)

    for _ in range(max(args.warmup, 3)):                 # >= 3: eager warm-up, capture, first replay
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed / args.steps * 1e3
    value = B * world * args.steps / elapsed
    metrics = eng.metrics_dict(weights)
    if args.dump_outputs and rank == 0:
        dump_step_outputs(model, eng, args.dump_outputs)

    # ---- roofline of the dominant kernel: HIP events around every GEMM main-kernel launch of 2 eager steps, recorded
    # by the library on the launch stream and keyed by kernel instantiation (the names rocprofv3 prints) -------------
    roof = None
    if args.full and not args.no_kernel_profile:
        def two_eager_steps():
            for _ in range(2):      # every rank runs them (they contain the collective); only rank 0 reports
                eng.train_step(x, mask, weights, hp["lr"], hp["wd"], hp["clip"], use_graph=False)
        prof = L.gemm_profile(two_eager_steps)
        if rank == 0:
            tot_t = sum(v[1] for v in prof.values())
            tot_f = sum(v[2] for v in prof.values())
            dom = max(prof, key=lambda k: prof[k][1])            # the instantiation with the largest summed time
            n, t, f = prof[dom]
            kname = L.gemm_kernel_name(dom)
            # the committed counter passes were taken on C2: per-launch bytes of another workload are not known
            traffic, traffic_src = pmc_traffic(kname) if args.workload == "c2" and not args.batch and not args.seq else (None, None)
            per_kernel = {L.gemm_kernel_name(k): {"launches_per_step": v[0] // 2, "avg_launch_us": round(v[1] / v[0] * 1e6, 2),
                                                  "achieved": round(v[2] / v[1] / 1e12, 2)}
                          for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}
            # The fraction is taken on the pipe that EXECUTES the kernel.  An x3 kernel computes each fp32 product with 6 bf16
            # MFMA products: `achieved` = 6 x ALGORITHMIC flops (2 M N K) / kernel time against the dense bf16 peak; the
            # fp32-equivalent rate (algorithmic flops / time) stands beside it as information, never as a fraction.
            x3 = L.gemm_kernel_is_x3(dom)
            mult, peak = (X3_PRODUCTS, BF16_MFMA_PEAK_TFLOPS) if x3 else (1, FP32_MFMA_PEAK_TFLOPS)
            roof = {"bound": "mfma", "kernel": kname, "achieved": round(mult * f / t / 1e12, 2),
                    "peak": peak, "unit": "TFLOP/s", "frac": round(mult * f / t / 1e12 / peak, 4),
                    "arithmetic": ("bf16 MFMA on exact 3-way splits of the fp32 operands: 6 bf16 products per fp32 product, fp32 "
                                   "accumulate; achieved = executed bf16 flops (6 x 2MNK) / time vs the dense bf16 peak" if x3
                                   else "fp32 MFMA"),
                    "fp32_equivalent": {"achieved": round(f / t / 1e12, 2), "unit": "TFLOP/s",
                                        "what": "algorithmic 2MNK / kernel time (fp32 MFMA peak is %.1f)" % FP32_MFMA_PEAK_TFLOPS},
                    "traffic": traffic, "traffic_source": traffic_src, "launches_per_step": n // 2,
                    "avg_launch_us": round(t / n * 1e6, 2), "gflop_per_launch": round(f / n / 1e9, 3),
                    "all_gemm_kernels": {"achieved_fp32_equivalent": round(tot_f / tot_t / 1e12, 2), "time_ms_per_step": round(tot_t / 2 * 1e3, 3),
                                         "gflop_per_step": round(tot_f / 2 / 1e9, 1), "per_kernel": per_kernel},
                    "step_level": {"gflop_per_sample": wl["gflop"], "unit": "TFLOP/s fp32-equivalent per GPU",
                                   "achieved": round(value / world * wl["gflop"] / 1e3, 2)}}

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(mp, weights, hp, B_cpu=min(B, 256), L=min(Lq, 64))

    if rank == 0:
        out = {"metric": "train images/sec @64x64x3 bs256 (curve tensors [B,64,6], SURVEY.md s0)", "value": round(value, 2),
               "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32", "gemm_arithmetic": ("bf16x3 exact split (6 products, fp32 accumulate)" if args.gemm == "x3"
                                                   else "native fp32 MFMA"),
               "data": "synthetic",
               "config": {"workload": f"{wl['desc']}; full train step (fwd+loss+bwd+clip+AdamW+EMA), dropout 0.1, "
                                      f"loss weights at epoch {BENCH_EPOCH}",
                          "per_gpu_batch": B, "global_batch": B * world, "seq_len": Lq, "parallelism": f"dp{world}",
                          "hipgraph": not args.no_graph, "params": int(sum(p.numel() for p in model.parameters()))},
               "loss": round(metrics["loss"], 6), "vq_loss": round(metrics["VQ_Loss"], 8),
               "recon_loss_xyz": round(metrics["Reconstruction_Loss_XYZ"], 6),
               "roofline": roof, "cpu_baseline": cpu}
        print(json.dumps(out), flush=True)
    if world > 1 or selftest:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
