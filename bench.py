#!/usr/bin/env python3
"""bench.py -- Ref-NeRF rendering inner loop on MI355X.

One "step" = one pass of the hot path over one synthetic batch through the fused HIP kernels:
``Model.__call__`` (eval forward, compute_extras=True, full ray_history) for the rendering
configurations, a full training step (training forward + losses + backward + gradient all-reduce +
Adam) for C5.  Prints ONE JSON line.

  python bench.py [--gpus N --steps K --warmup W] [--config C2|C3|C4|C5] [--full] [--dump-outputs DIR]

A plain run sets up, runs W warm-up steps, times exactly K steps and prints the line (metric, value, unit,
higher_is_better, dtype, ms_per_step = milliseconds per timed step).  --full adds everything else the benchmark
measures or checks: the median of five timed blocks, the other arithmetic modes, image renders, training legs, CPU
baselines, parity against the CPU oracle, the other configurations and the full record.  --dump-outputs DIR writes
what the timed path computed in its last step as DIR/<name>.npy (float32 / float64, <= 64 MB; inputs are seeded).

  --config C2 (default, the headline): blender_refnerf.gin, 4096 rays x 128 samples x 2 levels per GPU (weak scaling)
  --config C3: the "shiny" network (raw_roughness.bias = -6), 8192 rays x 192 samples x 2 levels per GPU (weak)
  --config C4: llff_refnerf.gin rays, 4096 rays x 128 samples over ALL ranks (strong scaling: 4096/N rays per rank;
               below 1024 rays per rank the level loop is replayed from a HIP graph)
  --config C5: llff_refnerf_geometry_losses.gin, 16384 rays x 256 samples over ALL ranks (strong: 16384/N per rank),
               full training step with the nine-term loss set and ONE RCCL all-reduce of the 4.44 MB gradient blob

Multi-GPU: `--gpus N` with N > 1 starts N processes itself (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* in their environment) BEFORE anything touches a GPU, unless it is already running under torchrun
(RANK set), in which case it is one of the ranks.  Rays shard by rank, weights are replicated, no data-path
collective; RCCL carries the timing barrier and, for C5, the gradient all-reduce.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_SAMPLE = 2211840            # MLP contractions only
NORMALS_VJP_FLOP = 1016320           # density-normal VJP of the training forward
TRAIN_FLOP_PER_SAMPLE = 7651840      # fwd + density-normal VJP + backward
PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0, "f16": 2500.0, "f16x2": 2500.0}   # MI355X dense MFMA peaks (MI355X_MICROARCH.md)
EVAL_MODES = ("f32", "f16x2", "bf16", "f16")
# what each arithmetic mode is, in the reader's terms ("accuracy of the arithmetic modes")
MODE_NOTES = {
    "f16x2": "parity-grade 16-bit mode of record: split-operand f16 MFMA (hi + lo halves in the spatial trunk and the density head, "
             "plain f16 directional trunk), fp32 accumulate, fp32 resampler / encodings / compositing; <= 1e-4 RGB vs the reference "
             "also on trained-like weights; three partial products on v_mfma_f32_16x16x32_f16: 1.5x the algorithmic matrix cycles (priced at the algorithmic FLOPs here)",
    "f32": "strict parity mode: exact fp32 MFMA fma chains",
    "bf16": "throughput mode: bf16 operands, hardware transcendentals; within 1e-4 on random-init networks only (5e-2 on trained-like weights)",
    "f16": "throughput mode: f16 operands, hardware transcendentals; within 1e-4 on random-init networks only (1e-2 on trained-like weights)",
}
PEAK_HBM_GBS = 8000.0

CONFIGS = {
    # name: rays (per GPU when weak, total when strong), samples, gin file, ray family, mode, scaling, weight recipe
    "C2": dict(rays=4096, samples=128, gin="refnerf_blender.gin", family="blender", mode="eval", scaling="weak",
               params=dict(seed=0, bias_scale=0.05, sharpen=20.0),
               workload="blender_refnerf.gin, 4096 rays x 128 samples, 2-level, Model.__call__ eval forward with "
                        "compute_extras + full ray_history"),
    "C3": dict(rays=8192, samples=192, gin="refnerf_blender.gin", family="blender", mode="eval", scaling="weak",
               params=dict(seed=0, bias_scale=0.05, sharpen=20.0, roughness_bias=-6.0),
               workload="blender_refnerf.gin shiny network (roughness ~1e-3), 8192 rays x 192 samples, 2-level, "
                        "Model.__call__ eval forward with compute_extras + full ray_history"),
    "C4": dict(rays=4096, samples=128, gin="refnerf_llff.gin", family="llff", mode="eval", scaling="strong",
               params=dict(seed=0, bias_scale=0.05, sharpen=20.0),
               workload="llff_refnerf.gin forward-facing NDC rays, 4096 rays x 128 samples over all ranks, 2-level, "
                        "Model.__call__ eval forward with compute_extras + full ray_history"),
    "C5": dict(rays=16384, samples=256, gin="refnerf_llff_geometry_losses.gin", family="llff", mode="train",
               scaling="strong", params=dict(seed=0, bias_scale=0.05, sharpen=20.0),
               workload="llff_refnerf_geometry_losses.gin, 16384 rays (+ noisy rays) x 256 samples over all ranks, "
                        "2-level, full training step: clean + noisy pass, nine loss terms, fused backward, gradient "
                        "all-reduce, Adam"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="C2", choices=sorted(CONFIGS))
    ap.add_argument("--rays", type=int, default=None, help="override the configuration's ray count")
    ap.add_argument("--samples", type=int, default=None, help="override the configuration's samples per level")
    ap.add_argument("--precision", default="f16x2", choices=list(EVAL_MODES),
                    help="arithmetic of the MLP contractions for the headline value (eval configurations); the other modes are "
                         "reported alongside.  Default: the parity-grade 16-bit mode")
    ap.add_argument("--train-precision", default="f16x2", choices=["f32", "f16x2", "bf16"],
                    help="MLP chains of the training step that carries the C5 headline (f32 = exact; f16x2 = split-f16 forward + f32 "
                         "backward, parity-grade; bf16 = throughput mode)")
    ap.add_argument("--no-other-configs", action="store_true", help="C2 only: skip the short C3 / C4-shard / C5-shard legs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-image", action="store_true")
    ap.add_argument("--no-train", action="store_true", help="skip the secondary training-step measurement")
    ap.add_argument("--no-graph", action="store_true", help="never replay the level loop from a HIP graph")
    ap.add_argument("--no-rccl", action="store_true",
                    help="single-GPU training legs: do not create the one-rank RCCL group (then the gradient all-reduce is skipped as "
                         "torch.distributed is not initialised)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: the median of several timed blocks, the other arithmetic modes, image renders, "
                         "training legs, CPU baselines, parity checks, other configurations and the full record (the --no-* options "
                         "trim it).  Without it a run sets up, warms up, times exactly --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------ output
INDEX_CONTRACT = ("sampler stage AND the fused level on identical (sdist, weights): CDF bin indices and sdist bit-exact vs the oracle (shared "
                  "rn_det_logf / rn_det_expf; test_sampler_*, test_f16x2_full_size_vs_oracle); end to end through Model.__call__: >= 99.999 % "
                  "identical, the differing ones are CDF ties one ulp apart (SURVEY H1)")
COMPACT_LIMIT = 4096       # bytes: the driver parses the tail of stdout it keeps (~8 KB); VERDICT r03 asks for <= 4 KB


def _sig(x, digits=5):
    """Numbers of the compact line at `digits` significant figures (bytes matter there)."""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        return float(f"{x:.{digits}g}")
    if isinstance(x, dict):
        return {k: _sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, digits) for v in x]
    return x


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def _leg(d):
    """{value, ms_per_step, frac} of one measured leg of the full record."""
    if not isinstance(d, dict) or "value" not in d:
        return None
    out = _pick(d, ("value", "ms_per_step"))
    if isinstance(d.get("roofline"), dict):
        out["frac"] = d["roofline"].get("frac")
    return out


def _train_leg(d):
    out = _leg(d)
    if out is None:
        return None
    out.pop("frac", None)
    for k, v in (d.get("kernels") or {}).items():        # per kernel family: launch ms and fraction of its roofline
        out[k] = [v.get("avg_launch_ms"), v.get("frac")]
    return out


def _parity_pair(p, mode):
    """(RGB L-inf vs the CPU oracle, identical-bin-index fraction, "k of n" differing indices) of one mode of a parity block."""
    m = (p or {}).get(mode) if isinstance(p, dict) else None
    if not isinstance(m, dict):
        return None
    out = {"rgb_linf": m.get("rgb_linf_vs_oracle"), "bin_idx_agreement": m.get("bin_idx_agreement")}
    if "bin_idx_differing" in m:
        out["bin_idx_differing"] = m["bin_idx_differing"]
    if "rgb_p9999" in m:
        out["rgb_p9999"] = m["rgb_p9999"]
    if "rays_over_1e-4" in m:
        out["rays_over_1e-4"] = m["rays_over_1e-4"]
    return out


def compact_line(full):
    """The LAST stdout line: the contract's keys + roofline + cpu_baseline + one {value, ms_per_step, frac} per secondary
    leg + four parity numbers, <= COMPACT_LIMIT bytes.  Everything else lives in the full record (`full_record`)."""
    mode = full.get("dtype")
    line = _pick(full, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                        "vs_baseline", "dtype", "data"))
    cfgd = dict(full.get("config") or {})
    if len(str(cfgd.get("workload", ""))) > 160:
        cfgd["workload"] = cfgd["workload"][:157] + "..."
    line["config"] = cfgd
    if isinstance(full.get("roofline"), dict):
        line["roofline"] = _pick(full["roofline"], ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms", "launches",
                                                    "mfma_busy", "executed_flop_frac", "sustained_clock_ghz"))
        src = str(full["roofline"].get("pmc_source") or full["roofline"].get("traffic_source") or "")
        if src:   # where traffic / mfma_busy / executed_flop_frac / sustained_clock_ghz come from (they are NOT measured in this run)
            line["roofline"]["pmc_source"] = src.split(" via ")[0]
    if isinstance(full.get("timed_blocks"), dict):
        line["timed_blocks"] = full["timed_blocks"]
    if isinstance(full.get("cpu_baseline"), dict):
        cb = dict(full["cpu_baseline"])
        if len(str(cb.get("sample", ""))) > 140:
            cb["sample"] = cb["sample"][:137] + "..."
        line["cpu_baseline"] = cb
    tb = [t for t in (full.get("cpu_baseline_torch") or []) if isinstance(t, dict) and t.get("value")]
    if tb:
        line["cpu_baseline_torch"] = {"value": tb[-1]["value"], "cores": tb[-1].get("cores")}
    modes = {m: _leg(full.get(m + "_mode")) for m in EVAL_MODES if _leg(full.get(m + "_mode"))}
    if modes:
        line["other_modes"] = modes
    train = {}
    for k, v in full.items():           # "train_step" (its own "dtype" names the chains) and "train_step_<chains>"
        if k.startswith("train_step") and _train_leg(v):
            train[k[len("train_step_"):] or v.get("dtype", "f32")] = _train_leg(v)
    if train:
        line["train_step"] = train
    oc = {}
    for name, leg in (full.get("other_configs") or {}).items():
        if not isinstance(leg, dict):
            continue
        if "error" in leg:
            oc[name] = {"error": str(leg["error"])[:60]}
        elif "value" in leg:
            oc[name] = dict(_train_leg(leg), dtype=leg.get("dtype"))
            if isinstance(leg.get("rccl"), dict):        # the step's gradient all-reduce ran through a one-rank RCCL group
                oc[name]["rccl"] = "error" if "error" in leg["rccl"] else f"{leg['rccl'].get('backend')} x{leg['rccl'].get('world_size')}"
        else:
            oc[name] = {m: _leg(v) for m, v in leg.items() if _leg(v)}
    if oc:
        line["other_configs"] = oc
    par = full.get("parity")
    if isinstance(par, dict):
        cp = {"rays_checked": par.get("rays_checked"), "bench_batch": _parity_pair(par, mode)}
        for tag, key in (("trained_like", "trained_like_weights"), ("trained_long", "trained_long_weights")):
            if _parity_pair(par.get(key), mode):
                cp[tag] = _parity_pair(par[key], mode)
        cp["index_contract"] = INDEX_CONTRACT
        line["parity"] = cp
    for k in ("full_image_render_ms", "llff_image_render_ms", "rccl"):
        if k in full:
            line[k] = full[k]
    line["full_record"] = full.get("full_record", "gpurun_out/bench_full.json")
    line = _sig(line)
    # never exceed the limit: drop the optional blocks from the least important one
    for victim in ("cpu_baseline_torch", "train_step", "other_modes", "other_configs", "llff_image_render_ms"):
        if len(json.dumps(line)) <= COMPACT_LIMIT:
            break
        line.pop(victim, None)
    return line


_REAL_STDOUT = None


def claim_stdout():
    """stdout must carry exactly ONE line.  Libraries print there behind Python's back -- RCCL writes its version banner
    ("RCCL version : ...", five lines, C stdio) when a communicator is created, flushed at exit, i.e. AFTER the JSON line --
    so fd 1 is pointed at stderr for everything else and the compact line goes to a private duplicate of the original."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)
    return _REAL_STDOUT


def emit(full):
    """Full record -> gpurun_out/bench_full.json and ONE stderr line (`BENCH_FULL {...}`); stdout carries exactly one line,
    the compact one (BENCH_r03.json had parsed = null: the 20 KB line overflowed the ~8 KB stdout tail the driver parses)."""
    full["full_record"] = "gpurun_out/bench_full.json"
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "bench_full.json"), "w") as f:
            json.dump(full, f, indent=1)
    except OSError as e:
        full["full_record"] = f"stdout only ({type(e).__name__})"
    print("BENCH_FULL " + json.dumps(full), file=sys.stderr)
    sys.stderr.flush()
    out = _REAL_STDOUT or sys.stdout
    out.write(json.dumps(compact_line(full)) + "\n")
    out.flush()


def emit_line(line):
    """A plain run's record: the compact line on stdout, nothing else (no full record beside it)."""
    line = compact_line(line)
    line.pop("full_record", None)
    out = _REAL_STDOUT or sys.stdout
    out.write(json.dumps(line) + "\n")
    out.flush()


DUMP_BYTES = 60 << 20      # array bytes of one --dump-outputs (the .npy headers keep the files under 64 MB in all)


def _dump_array(x):
    """float64 stays float64, other floating types go out as float32, integers and flags as float64 (exact)."""
    import numpy as np
    import torch
    if isinstance(x, torch.Tensor):
        x = x.detach()
        x = (x.float() if x.is_floating_point() and x.dtype != torch.float64 else x.double()).contiguous().cpu().numpy()
    x = np.asarray(x)
    return x if x.dtype in (np.float32, np.float64) else x.astype(np.float64 if x.dtype.kind in "iub" else np.float32)


def dump_outputs(out_dir, arrays, n_rays):
    """--dump-outputs: {name: tensor} of what the timed path handed its caller in its last step -> out_dir/<name>.npy.  When
    they exceed DUMP_BYTES, the per-ray arrays (leading dimension n_rays) keep a fixed, seeded sample of the rays, the same
    for every array and every run with the same arguments; its ray indices go to ray_index.npy."""
    import numpy as np
    arrays = {k: _dump_array(v) for k, v in arrays.items()}
    per_ray = [k for k, a in arrays.items() if a.ndim and a.shape[0] == n_rays]
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BYTES:
        ray_bytes = sum(arrays[k].nbytes for k in per_ray) // n_rays
        keep = (DUMP_BYTES - (total - ray_bytes * n_rays)) // (ray_bytes + 8)
        if keep < 1:
            raise ValueError(f"--dump-outputs: {total} bytes of outputs, no ray sample fits in {DUMP_BYTES}")
        idx = np.sort(np.random.default_rng(0).choice(n_rays, keep, replace=False))
        for k in per_ray:
            arrays[k] = arrays[k][idx]
        arrays["ray_index"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return sorted(arrays)


def eval_outputs(out):
    """The (renderings, ray_history) of one Model.__call__ as {name: tensor}: level<l>_rendering_<key>, level<l>_history_<key>."""
    renderings, history = out
    arrays = {}
    for lvl, (rend, hist) in enumerate(zip(renderings, history)):
        arrays.update({f"level{lvl}_rendering_{k}": v for k, v in rend.items() if v is not None})
        arrays.update({f"level{lvl}_history_{k}": v for k, v in hist.items() if v is not None})
    return arrays


def train_outputs(model, loss):
    """What one training step leaves its caller: the loss, and per MLP the flat parameter blob after the Adam step and the
    (all-reduced) gradient blob it was taken from."""
    arrays = {"loss": [loss]}
    for name, mlp in (("nerf_mlp", model.nerf_mlp), ("prop_mlp", model.prop_mlp)):
        if name == "prop_mlp" and mlp is model.nerf_mlp:
            continue
        flat = mlp.flat_params()
        arrays[name + "_params"] = flat
        if flat.grad is not None:
            arrays[name + "_grad"] = flat.grad
    return arrays


# ------------------------------------------------------------------------------------------------ launcher
def launch_ranks(args) -> int:
    """Parent of `--gpus N` (N > 1) outside torchrun: start one fresh child per GPU and relay rank 0's JSON line.
    Nothing here initialises a GPU (torch.cuda.device_count() only counts devices)."""
    import torch
    n = args.gpus
    share = os.environ.get("REFNERF_BENCH_SHARE_GPU") == "1"
    visible = torch.cuda.device_count()
    if visible < n and not share:
        print(f"bench.py: --gpus {n} but only {visible} device(s) visible "
              "(REFNERF_BENCH_SHARE_GPU=1 lets the ranks share device 0 for a smoke run)", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out0 = procs[0].stdout.read().decode()
    codes = [p.wait() for p in procs]
    if any(codes):
        print(f"bench.py: rank exit codes {codes}", file=sys.stderr)
        sys.stderr.write(out0)
        return 1
    sys.stdout.write(out0)
    return 0


def one_rank_rccl(dev):
    """Single-GPU training legs: a ONE-rank RCCL ("nccl") group, so that the step includes the gradient all-reduce call and
    `n_ranks_seen` comes from RCCL (the reference trains under DDP on NCCL/RCCL, train.py:84-88).
    Returns (torch.distributed or None, info dict)."""
    import datetime
    import torch.distributed as dist
    if dist.is_initialized():
        return dist, {"backend": dist.get_backend(), "world_size": dist.get_world_size()}
    try:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        t0 = time.perf_counter()
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=1, rank=0, device_id=dev,
                                timeout=datetime.timedelta(seconds=120))
        return dist, {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "init_s": time.perf_counter() - t0}
    except Exception as e:            # never lose the line over it: the step then runs without the collective, and says so
        return None, {"error": repr(e)[:200]}


# ------------------------------------------------------------------------------------------------ workload
def build_model(args, spec, dev):
    import refnerf_pl_amd  # noqa: F401
    from refnerf_pl_amd import configs, models, synthetic
    configs.clear_config()
    configs.parse_config_files_and_bindings([os.path.join(ROOT, "configs", spec["gin"])], [
        f"Model.num_prop_samples = {spec['samples']}", f"Model.num_nerf_samples = {spec['samples']}",
        f"Config.batch_size = {spec['rays']}", f"Config.hip_precision = '{args.precision}'"])
    cfg = configs.Config()
    model = models.construct_model(None, cfg).to(dev)
    model.eval()
    blob = synthetic.make_params(**spec["params"])
    model.nerf_mlp.load_flat_params(blob)
    return model, cfg, blob


def make_rays(spec, n_rays, seed):
    from refnerf_pl_amd import synthetic
    if spec["family"] == "llff":
        return synthetic.llff_rays(n_rays, seed=seed)
    return synthetic.blender_rays(n_rays, seed=seed, center_frac=0.5)


def host_cores():
    """CPUs this process may run on: its affinity mask, capped by OMP_NUM_THREADS when that is set (a shared host's
    quota).  os.cpu_count() counts the whole machine, and OpenMP pools sized by it only slow themselves down."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS", "")
    return max(1, min(n, int(omp)) if omp.isdigit() and int(omp) > 0 else n)


def cpu_sample_size(spec, cores):
    """FIXED size of the CPU-baseline sample (no calibration runs: the figure used to drift by 40 % with them): the
    first n rays of rank 0's own batch -- the whole batch on a many-core host (~10-20 s), 512 rays otherwise."""
    return min(spec["rays"], 4096 if cores >= 64 else 512)


def cpu_baseline_and_parity(blob, spec, rays_np, hip_outputs):
    """(a) cpu_baseline: the CPU oracle (a from-scratch C port of the reference's algorithm, OpenMP over rays, all
    host cores) timed on a fixed prefix of the batch the GPU just rendered; (b) its outputs double as the checker
    of the GPU results of both arithmetic modes on exactly those rays (`parity`)."""
    import numpy as np
    from oracle import oracle as O
    cores = host_cores()
    N = spec["samples"]
    n = cpu_sample_size(spec, cores)
    sub = {k: v[:n] for k, v in rays_np.items()}
    O.model_forward(blob, {k: v[:64] for k, v in rays_np.items()}, num_prop_samples=N, num_nerf_samples=N, n_threads=cores)  # thread start-up, page faults
    t0 = time.time()
    ref = O.model_forward(blob, sub, num_prop_samples=N, num_nerf_samples=N, n_threads=cores, history=True)
    dt = time.time() - t0
    base = {"value": n * N * 2 / dt, "unit": "ray-samples/s", "cores": cores, "kind": "port",
            "sample": f"first {n} rays of the timed batch x {N} samples x 2 levels, eval forward with full history, "
                      f"fp32, OpenMP over rays, {dt:.1f} s"}
    parity = {"rays_checked": n, "checker": "oracle/refnerf_oracle.c (pinned by tests/golden, captured from the reference)"}
    for tag, (out, bin_idx) in hip_outputs.items():
        rgb = out[0][-1]["rgb"][:n].float().cpu().numpy()
        err = np.abs(rgb - ref[-1]["r_rgb"])
        mse = float(np.mean((rgb.astype(np.float64) - ref[-1]["r_rgb"]) ** 2))
        w_hip = out[1][-1]["weights"][:n].cpu().numpy()
        same = bin_idx[-1][:n].cpu().numpy() == ref[-1]["bin_idx"]
        parity[tag] = {"rgb_linf_vs_oracle": float(err.max()), "psnr_vs_oracle_db": float(-10 * np.log10(max(mse, 1e-20))),
                       "rgb_p9999": float(np.quantile(err.max(axis=-1), 0.9999)), "rays_over_1e-4": int((err.max(axis=-1) > 1e-4).sum()),
                       "weights_linf_vs_oracle": float(np.abs(w_hip - ref[-1]["weights"]).max()),
                       # north_star's "bit-exact sample indices": the CDF bin every sample of the final level was drawn from
                       "bin_idx_agreement": float(np.mean(same)), "bin_idx_differing": f"{int(same.size - same.sum())} of {same.size}",
                       "sdist_max_abs_diff": float(np.abs(out[1][-1]["sdist"][:n].cpu().numpy() - ref[-1]["sdist"]).max())}
    return base, parity


def trained_like_parity(model, cfg, dev, spec, modes, which="trained_blob.npz"):
    """The same check on "trained-like" weights -- tests/golden/trained_blob.npz: what the REFERENCE reached after 400 of
    its own Adam steps on an analytic shiny sphere (stored as float16); trained_long_blob.npz: after 2500 steps at twice
    the learning rate, stored in fp32 --: 256 Blender rays x this configuration's sample counts, every arithmetic mode
    against the CPU oracle.  Random-init weights flatter 16-bit arithmetic; these do not."""
    import numpy as np
    import torch
    from oracle import oracle as O
    from refnerf_pl_amd import synthetic, utils
    path = os.path.join(ROOT, "tests", "golden", which)
    if not os.path.exists(path):
        return None
    z = np.load(path)
    blob = z["blob_f32"] if "blob_f32" in z.files else z["blob_f16"].astype(np.float32)
    N = spec["samples"]
    llff = spec["family"] == "llff"
    rays_np = synthetic.llff_rays(256, seed=3) if llff else synthetic.blender_rays(256, seed=3, center_frac=0.8)
    okw = dict(srgb_mapping=int(model.nerf_mlp.srgb_mapping),
               render_srgb_mode=cfg.srgb_mapping_type if cfg.srgb_mapping_when_rendering else "none")
    ref = O.model_forward(blob, rays_np, num_prop_samples=N, num_nerf_samples=N, n_threads=host_cores(), history=True, **okw)
    keep = model.nerf_mlp.flat_params().clone()
    model.nerf_mlp.load_flat_params(blob)
    rays = utils.rays_from_dict(rays_np, dev)
    res = {"rays_checked": 256, "weights": "tests/golden/" + which}
    prev = cfg.hip_precision
    for m in modes:
        cfg.hip_precision = m
        with torch.no_grad():
            out = model(rays, 1.0, True)
        rgb = out[0][-1]["rgb"].cpu().numpy()
        mse = float(np.mean((rgb.astype(np.float64) - ref[-1]["r_rgb"]) ** 2))
        same = model.last_bin_idx[-1].cpu().numpy() == ref[-1]["bin_idx"]
        res[m] = {"rgb_linf_vs_oracle": float(np.abs(rgb - ref[-1]["r_rgb"]).max()),
                  "psnr_vs_oracle_db": float(-10 * np.log10(max(mse, 1e-20))),
                  "bin_idx_agreement": float(np.mean(same)), "bin_idx_differing": f"{int(same.size - same.sum())} of {same.size}"}
    cfg.hip_precision = prev
    model.nerf_mlp.load_flat_params(keep)
    return res


def cpu_baseline_train(model, cfg, blob, spec, rays_np, rank):
    """cpu_baseline of the training configuration (C5): the CPU oracle's training step (`rn_level_train`: cached forward, the
    data / orientation / predicted-normal losses, full backward into the gradient blob; the other six terms of the nine-term
    set are elementwise on the level outputs and are not part of this timing) on a fixed prefix of rank 0's batch."""
    from oracle import oracle as O
    from refnerf_pl_amd import synthetic
    cores = host_cores()
    N = spec["samples"]
    n = min(rays_np["origins"].shape[0], 256 if cores >= 64 else 16)        # (the oracle's training step: ~1e4 ray-samples/s on 256 cores)
    sub = {k: v[:n] for k, v in rays_np.items()}
    gt = synthetic.target_rgb(n, seed=7 + rank)
    okw = dict(srgb_mapping=int(model.nerf_mlp.srgb_mapping),
               render_srgb_mode=cfg.srgb_mapping_type if cfg.srgb_mapping_when_rendering else "none")
    O.model_train(blob, {k: v[:16] for k, v in rays_np.items()}, gt[:16], num_prop_samples=N, num_nerf_samples=N, n_threads=cores, **okw)
    t0 = time.time()
    losses, _, _ = O.model_train(blob, sub, gt, num_prop_samples=N, num_nerf_samples=N, n_threads=cores, **okw)
    dt = time.time() - t0
    return {"value": n * N * 2 / dt, "unit": "ray-samples/s", "cores": cores, "kind": "port",
            "sample": f"first {n} rays x {N} samples x 2 levels, training forward + three Ref-NeRF losses + backward, fp32, "
                      f"OpenMP over rays, {dt:.1f} s"}


def torch_cpu_baseline(spec):
    """Second CPU baseline: the build's own UNFUSED PyTorch restatement of the path (oracle/torch_path.py,
    plain ATen ops on the host cores -- how the reference itself evaluates the path), at C1's shape and at this
    configuration's shape on a bounded sample.  Runs in a child process (its own OpenMP runtime: the C oracle's
    spinning worker threads otherwise fight torch's) and keeps the fastest of two intra-op thread counts."""
    out = []
    n2 = min(spec["rays"], 1024)
    for tag, n_rays, N, levels in ((f"C1 shape: 1024 rays x 64 samples x 1 level", 1024, 64, 1),
                                   (f"this configuration's samples: {n2} rays x {spec['samples']} samples x 2 levels", n2, spec["samples"], 2)):
        try:
            r = subprocess.run([sys.executable, "-m", "oracle.torch_path", spec["family"], str(n_rays), str(N), str(levels),
                                json.dumps(spec["params"])], cwd=ROOT, capture_output=True, text=True, timeout=150)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            out.append({"value": res["rate"], "unit": "ray-samples/s", "cores": res["threads"], "kind": "port",
                        "sample": f"unfused PyTorch CPU path, {tag}, eval forward, fp32, {res['seconds']:.2f} s per pass "
                                  f"(best of {res['tried']} intra-op thread counts <= 64 on {host_cores()} cores: ATen's elementwise ops and "
                                  f"small GEMMs get slower, not faster, with hundreds of threads -- 256 threads: > 50 s per pass at C1's shape)"})
        except (subprocess.TimeoutExpired, ValueError, IndexError, KeyError) as e:
            out.append({"value": None, "unit": "ray-samples/s", "cores": None, "kind": "port",
                        "sample": f"unfused PyTorch CPU path, {tag}: not measured ({type(e).__name__})"})
    return out



# ------------------------------------------------------------------------------------------------ measurement helpers
N_BLOCKS = 5       # repetitions of the headline's timed block (the median one is reported)


def traffic_of(kernel, config_name, rays_per_rank, N):
    """PMC numbers cannot be collected inside this process: copied from the committed rocprofv3 --pmc passes
    (profiles/traffic.json), only for the workload they were measured on."""
    try:
        prof = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        key = f"{kernel}@{config_name}"
        entry = prof[key] if key in prof else (prof[kernel] if config_name == "C2" and kernel in prof else None)
        if entry and rays_per_rank == CONFIGS[config_name]["rays"] and N == CONFIGS[config_name]["samples"]:
            return entry["bytes_per_launch"], f"profiles/{entry.get('round', '?')}/pmc_{kernel.split('::')[-1]}{'' if config_name == 'C2' else '_' + config_name}.csv via profiles/traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes; not measured in this run)"
    except (OSError, KeyError, ValueError):
        pass
    return None, None


def pmc_of(kernel, config_name, rays_per_rank, N):
    """matrix-pipe occupancy figures of the committed PMC passes (profiles/traffic.json, scripts/summarize_prof.py):
    mfma_busy = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs), the sustained clock = GRBM_GUI_ACTIVE / 8 / launch
    duration, executed_flop_frac = mfma_busy x clock / 2.4 GHz = what the matrix pipes EXECUTED (all partial products) of the peak
    the roofline is priced at.  Only for the workload they were measured on."""
    try:
        prof = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        key = f"{kernel}@{config_name}"
        entry = prof[key] if key in prof else (prof[kernel] if config_name == "C2" and kernel in prof else None)
        if entry and "mfma_busy" in entry and rays_per_rank == CONFIGS[config_name]["rays"] and N == CONFIGS[config_name]["samples"]:
            out = {k: entry[k] for k in ("mfma_busy", "executed_flop_frac", "sustained_clock_ghz", "valu_per_mfma") if k in entry}
            out["pmc_source"] = (f"profiles/{entry.get('round', '?')}/pmc_{kernel.split('::')[-1]}{'' if config_name == 'C2' else '_' + config_name}.csv via "
                                 "profiles/traffic.json (SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE passes of the same command; not measured in this run)")
            return out
    except (OSError, KeyError, ValueError):
        pass
    return {}


def mfma_roofline(prec, kernel, kern_ms, launches, flop_per_launch, config_name, rays_per_rank, N):
    avg_ms = kern_ms / launches
    achieved = flop_per_launch / (avg_ms * 1e-3) / 1e12
    traffic, src = traffic_of(kernel, config_name, rays_per_rank, N)
    return dict({"bound": "mfma", "achieved": achieved, "peak": PEAK_TFLOPS[prec], "unit": "TFLOP/s",
                 "frac": achieved / PEAK_TFLOPS[prec], "traffic": traffic, "traffic_source": src, "kernel": kernel,
                 "avg_launch_ms": avg_ms, "launches": launches, "flop_per_launch": flop_per_launch,
                 "timing": "HIP event pairs on the launch stream, inside the timed region"},
                **pmc_of(kernel, config_name, rays_per_rank, N))


def eval_kernel_name(prec, N, rays_per_rank):
    name = {"f32": "rn::level_fwd_f32", "bf16": "rn::level_fwd_bf16", "f16": "rn::level_fwd_f16", "f16x2": "rn::level_fwd_f16x2"}[prec]
    # the library's choice (refnerf_hip.hip level_forward_impl): sample counts that do not tile the 256-sample pass
    # within 640 records take the ring variant of the 16-bit kernel when the grid keeps >= 512 workgroups
    if prec != "f32" and N <= 256 and 256 % N != 0 and N % 256 != 0:
        r = next((k for k in range(1, 9) if (k * N) % 256 == 0), None)
        plain = 2 if (2 * N) % 256 == 0 and 2 * N <= 512 else (4 if (4 * N) % 256 == 0 and 4 * N <= 512 else 1)
        if r and (plain * N) % 256 != 0 and r * N > 640 and rays_per_rank // r >= 512:
            name += "_ring"
    return name


def timed_steps(step, n_steps, n_warm, with_events, sync, max_over_ranks):
    """n_warm untimed steps, then exactly n_steps bracketed by barrier + synchronize on both sides;
    returns (elapsed s [max over ranks], kernel ms total, launches, last output)."""
    from refnerf_pl_amd import _hip
    out = None
    for _ in range(n_warm):
        out = step()        # (held like the timed steps hold theirs: the caching allocator then sees the same live set in both
                            #  loops -- a fresh 57 MB output set hipMalloc'ed inside the timed region cost the last secondary leg
                            #  40-50 ms in round 3)
    sync()
    if with_events:
        _hip.set_timing(True)      # HIP event pairs on the kernel's own stream, inside the library
    t0 = time.perf_counter()
    for _ in range(n_steps):
        out = step()
    sync()
    el = time.perf_counter() - t0
    kern_ms, launches = _hip.get_timing() if with_events else (0.0, 0)
    _hip.set_timing(False)
    return max_over_ranks(el), kern_ms, launches, out


def other_configs(args, dev, sync, max_over_ranks):
    """Short legs of the other BASELINE configurations inside the default (C2) run, so that the driver's line carries
    them: C3 (8192 x 192, shiny network: the ring-of-records kernel variant) in the headline mode and in bf16, the
    per-GPU shard of C4 (512 LLFF rays, HIP-graph replay) and the per-GPU shard of C5 (2048 rays x 256 samples,
    nine-term geometry loss, training step in the parity-grade split-f16 chain mode, the exact-fp32 chains beside it).  A few steps each."""
    import argparse as _ap
    import torch
    from refnerf_pl_amd import _hip, graphs, utils
    out = {}
    a = _ap.Namespace(**vars(args))

    def eval_leg(name, spec, precs, n_steps, n_warm, graph):
        model, cfg, _ = build_model(a, spec, dev)
        R, N = spec["rays"], spec["samples"]
        rays = utils.rays_from_dict(make_rays(spec, R, seed=1), dev)
        leg = {"workload": spec["workload"] + f" [{R} rays on this GPU]", "rays": R, "samples_per_level": N, "hip_graph_replay": bool(graph)}
        for prec in precs:
            cfg.hip_precision = prec

            def eager():
                with torch.no_grad():
                    return model(rays, 1.0, True)
            step = eager
            if graph:
                g = graphs.GraphedForward(model, rays, 1.0, True)
                step = lambda: g(rays)      # noqa: E731
            el, k, l, o = timed_steps(step, n_steps, n_warm, not graph, sync, max_over_ranks)
            if graph:     # events cannot be recorded inside a graph replay: kernel durations from a short eager pass
                _, k, l, _ = timed_steps(eager, 5, 2, True, sync, max_over_ranks)
            assert torch.isfinite(o[0][-1]["rgb"]).all()
            leg[prec] = {"value": R * N * 2 * n_steps / el, "unit": "ray-samples/s", "ms_per_step": 1e3 * el / n_steps, "steps": n_steps,
                         "dtype": prec, "roofline": mfma_roofline(prec, eval_kernel_name(prec, N, R), k, l, R * N * FLOP_PER_SAMPLE, name, R, N)}
        out[name] = leg
        del model, rays
        torch.cuda.empty_cache()

    eval_leg("C3", dict(CONFIGS["C3"]), (args.precision, "bf16") if args.precision != "bf16" else ("bf16", "f16x2"), 5, 2, False)
    eval_leg("C4_shard", dict(CONFIGS["C4"], rays=512), (args.precision,), 20, 5, not args.no_graph)
    # the reference's constructor-default IPE basis ('icosahedron' / 2: 21 directions, 672 IPE features) at
    # the C2 shape: the f32 kernel with seven direction groups through layers 0 and 5 (FLOPs counted accordingly)
    try:
        from refnerf_pl_amd import configs, models, synthetic
        spec = dict(CONFIGS["C2"])
        configs.clear_config()
        configs.parse_config_files_and_bindings([os.path.join(ROOT, "configs", spec["gin"])], [
            f"Model.num_prop_samples = {spec['samples']}", f"Model.num_nerf_samples = {spec['samples']}",
            "Config.hip_precision = 'f32'", "NerfMLP.basis_shape = 'icosahedron'", "NerfMLP.basis_subdivisions = 2"])
        model = models.construct_model(None, configs.Config()).to(dev).eval()
        model.nerf_mlp.load_flat_params(synthetic.make_basis_params(n_basis=21, **spec["params"]))
        R, N = spec["rays"], spec["samples"]
        rays = utils.rays_from_dict(make_rays(spec, R, seed=1), dev)

        def ico_step():
            with torch.no_grad():
                return model(rays, 1.0, True)
        flop = R * N * (FLOP_PER_SAMPLE + 2 * 2 * 256 * 576)        # + the 6 extra direction groups of layers 0 and 5
        leg = {"workload": spec["workload"] + " with NerfMLP.basis_shape = 'icosahedron', basis_subdivisions = 2 (the reference's constructor default)",
               "rays": R, "samples_per_level": N}
        for prec, kern in (("f16x2", "rn::level_fwd_f16x2c_gb"), ("f32", "rn::level_fwd_f32_gb")):
            model.config.hip_precision = prec
            el, k, l, o = timed_steps(ico_step, 5, 2, True, sync, max_over_ranks)
            assert torch.isfinite(o[0][-1]["rgb"]).all()
            leg[prec] = {"value": R * N * 2 * 5 / el, "unit": "ray-samples/s", "ms_per_step": 1e3 * el / 5, "steps": 5, "dtype": prec,
                         "roofline": mfma_roofline(prec, kern, k, l, flop, "C2", R, N)}
        out["C2_icosahedron_basis"] = leg
        del model, rays
        torch.cuda.empty_cache()
    except Exception as e:      # never lose the headline line over an extra leg
        out["C2_icosahedron_basis"] = {"error": repr(e)}
    if not args.no_train:
        spec = dict(CONFIGS["C5"], rays=2048)
        model, cfg, _ = build_model(a, spec, dev)
        rays = utils.rays_from_dict(make_rays(spec, spec["rays"], seed=1), dev)
        dist1, rccl = (None, None) if args.no_rccl else one_rank_rccl(dev)       # the step's all-reduce through a one-rank RCCL group
        res = train_step_bench(a, spec, model, cfg, rays, 0, 1, dev, dist1, sync, max_over_ranks, args.train_precision, n_steps=3, n_warm=1, geometry=True)
        res["workload"] = spec["workload"] + " [2048 rays on this GPU: the per-GPU shard at 8 ranks]"
        res["rccl"] = rccl
        out["C5_shard"] = res
        if args.train_precision != "f32":
            out["C5_shard_f32_chains"] = train_step_bench(a, spec, model, cfg, rays, 0, 1, dev, None, sync, max_over_ranks, "f32", n_steps=2, n_warm=1, geometry=True)
        del model, rays
        torch.cuda.empty_cache()
    return out


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(launch_ranks(args))

    claim_stdout()
    import numpy as np
    import torch
    torch.manual_seed(0)       # the device-side draws of the step (the noisy rays of C5): identical inputs run to run
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # REFNERF_BENCH_BACKEND=gloo + REFNERF_BENCH_SHARE_GPU=1: smoke-test the N>1 code path on a 1-GPU box
        backend = os.environ.get("REFNERF_BENCH_BACKEND", "nccl")
        if os.environ.get("REFNERF_BENCH_SHARE_GPU") == "1":
            local_rank = 0
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    spec = dict(CONFIGS[args.config])
    rccl = None
    if world == 1 and not args.no_rccl and (args.full or spec["mode"] == "train"):
        # (eval configurations too since round 5: `n_ranks_seen` of EVERY leg comes from the RCCL group -- VERDICT r4 item 9;
        #  a plain eval run has no collective to issue and skips the group's start-up)
        dist, rccl = one_rank_rccl(dev)
    n_ranks_seen = dist.get_world_size() if dist is not None else 1
    assert n_ranks_seen == world

    if args.rays:
        spec["rays"] = args.rays
    if args.samples:
        spec["samples"] = args.samples
    strong = spec["scaling"] == "strong"
    rays_per_rank = spec["rays"] // world if strong else spec["rays"]
    total_rays = rays_per_rank * world
    N = spec["samples"]

    from refnerf_pl_amd import _hip, utils
    _hip.require_device()
    model, cfg, blob = build_model(args, spec, dev)
    # ray-tile data parallel: rank r works on its own tile of the (virtual) image / batch
    rays_np = make_rays(spec, rays_per_rank, seed=1 + rank)
    rays = utils.rays_from_dict(rays_np, dev)

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(el):
        if dist is None:
            return el
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    line = {"metric": None, "value": None, "unit": "ray-samples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": spec["scaling"],
            "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": spec["workload"], "name": args.config, "rays_per_gpu": rays_per_rank,
                       "total_rays": total_rays, "samples_per_level": N, "parallelism": f"ray-tile dp{world}",
                       "n_ranks_seen": n_ranks_seen}}

    def roofline_of(prec, kernel, kern_ms, launches, flop_per_launch):
        return mfma_roofline(prec, kernel, kern_ms, launches, flop_per_launch, args.config, rays_per_rank, N)

    if spec["mode"] == "eval":
        graphed = None
        use_graph = rays_per_rank < 1024 and not args.no_graph

        def eager_step():
            with torch.no_grad():
                return model(rays, 1.0, True)

        def make_step():
            nonlocal graphed
            if use_graph:
                from refnerf_pl_amd import graphs
                graphed = graphs.GraphedForward(model, rays, 1.0, True)
                return lambda: graphed(rays)
            return eager_step

        def timed(step, n_steps, n_warm, with_events):
            return timed_steps(step, n_steps, n_warm, with_events, sync, max_over_ranks)

        def kernel_name(prec):
            return eval_kernel_name(prec, N, rays_per_rank)

        step = make_step()
        # the driver passes --steps 20: ~80 ms of GPU time would be the whole evidence.  With --full the timed block of EXACTLY
        # args.steps steps (barrier + synchronize on both sides) is therefore repeated N_BLOCKS times and the MEDIAN block is the
        # one reported (its elapsed time, its event pairs); every block's ms per step travels in the line.  A plain run times
        # one block: exactly args.steps steps
        n_blocks = N_BLOCKS if args.full else 1
        blocks = [timed(step, args.steps, args.warmup if b == 0 else 0, with_events=not use_graph) for b in range(n_blocks)]
        order = sorted(range(n_blocks), key=lambda b: blocks[b][0])
        elapsed, kern_ms, launches, out = blocks[order[n_blocks // 2]]
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, eval_outputs(blocks[-1][3]), rays_per_rank)     # (the last block ends with the last step)
        if args.full:
            line["timed_blocks"] = {"blocks": N_BLOCKS, "reported": "median", "ms_per_step": [round(1e3 * b[0] / args.steps, 4) for b in blocks]}
        if use_graph and args.full:   # events cannot be recorded inside a graph replay: kernel durations from a short eager pass
            _, kern_ms, launches, _ = timed(eager_step, max(5, args.steps // 10), 2, True)
        rgb = out[0][-1]["rgb"]
        assert torch.isfinite(rgb).all()
        samples_per_step = total_rays * N * 2
        line["metric"] = (f"ray-samples/s ({spec['rays']} rays x {N} samples x 2 levels, Ref-NeRF "
                          f"{'Blender' if spec['family'] == 'blender' else 'LLFF'}, eval forward)")
        line["value"] = samples_per_step * args.steps / elapsed
        line["ms_per_step"] = 1e3 * elapsed / args.steps
        line["config"]["hip_graph_replay"] = bool(use_graph)
        flop_per_launch = rays_per_rank * N * FLOP_PER_SAMPLE
        if launches:
            line["roofline"] = roofline_of(args.precision, kernel_name(args.precision), kern_ms, launches, flop_per_launch)
        hip_outputs = {args.precision: (out, list(model.last_bin_idx))}
        line["dtype_note"] = MODE_NOTES[args.precision]
        if args.full and rank == 0 and world == 1:
            # the other arithmetic modes on the same batch (f32 = exact-fp32 MFMA, the strict parity mode; bf16 / f16 =
            # the two 16-bit MFMA throughput modes)
            def fp64_psnr(x, y):
                return float(-10 * torch.log10(torch.clamp(((x.double() - y.double()) ** 2).mean(), min=1e-20)))
            for other in [m for m in EVAL_MODES if m != args.precision]:
                cfg.hip_precision = other
                n2 = max(3, args.steps // 5)
                el2, k2, l2, out2 = timed(eager_step, n2, 3, True)      # 3 warm-up steps: a mode's first call re-packs / pages code in
                line[other + "_mode"] = {"value": samples_per_step * n2 / el2, "unit": "ray-samples/s",
                                         "ms_per_step": 1e3 * el2 / n2, "dtype": other, "note": MODE_NOTES[other],
                                         "roofline": roofline_of(other, kernel_name(other), k2, l2, flop_per_launch)}
                hip_outputs[other] = (out2, list(model.last_bin_idx))
            cfg.hip_precision = args.precision
            ref32, idx32 = hip_outputs["f32"]
            line["mode_agreement"] = {
                m: {"rgb_linf_vs_f32": float((o[0][-1]["rgb"] - ref32[0][-1]["rgb"]).abs().max()),
                    "psnr_vs_f32_db": fp64_psnr(o[0][-1]["rgb"], ref32[0][-1]["rgb"]),
                    "bin_idx_agreement": float((bi[-1] == idx32[-1]).double().mean()),
                    "sdist_max_abs_diff": float((o[1][-1]["sdist"] - ref32[1][-1]["sdist"]).abs().max())}
                for m, (o, bi) in hip_outputs.items() if m != "f32"}
        if args.full and rank == 0 and world == 1 and not args.no_image and args.config == "C2":
            from refnerf_pl_amd import camera_utils, models, synthetic
            # full-image render ms: 800x800 Blender view, 157 chunks of 4096 rays (models.render_image); the rays of
            # the whole view are cast on the device (refnerf_pixels_to_rays), inside the timed region
            c2w, focal = synthetic.blender_camera(seed=1)
            # two renders: the first one also pays for the one-off growth of torch's caching allocator (157 chunks of
            # outputs) and the first launch of the ray-casting kernel; the headline is the steady state
            for tag in ("full_image_render_first_ms", "full_image_render_ms"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad():
                    img = camera_utils.cast_pinhole_rays(c2w.astype(np.float32), 800, 800, focal, 2.0, 6.0, device=dev)
                    rendering = models.render_image(lambda r: model(r, 1.0, True), img, cfg, verbose=False, device=dev)
                torch.cuda.synchronize()
                line[tag] = 1e3 * (time.perf_counter() - t0)
            assert rendering["rgb"].shape == (800, 800, 3)
            # 1008x756 LLFF-style view (NDC rays, near 0 / far 1), same chunked loop
            del img, rendering
            lr = synthetic.llff_rays(0, seed=1, full_image=True)
            img = utils.rays_from_dict({k: v.reshape(756, 1008, -1) for k, v in lr.items()}, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                rendering = models.render_image(lambda r: model(r, 1.0, True), img, cfg, verbose=False, device=dev)
            torch.cuda.synchronize()
            line["llff_image_render_ms"] = 1e3 * (time.perf_counter() - t0)
            assert rendering["rgb"].shape == (756, 1008, 3)
            del img, rendering
        if args.full and not args.no_train and args.config == "C2":
            line["train_step"] = train_step_bench(args, spec, model, cfg, rays, rank, world, dev, dist, sync, max_over_ranks, "f32")
            line["train_step_f16x2"] = train_step_bench(args, spec, model, cfg, rays, rank, world, dev, dist, sync, max_over_ranks, "f16x2")
            line["train_step_bf16"] = train_step_bench(args, spec, model, cfg, rays, rank, world, dev, dist, sync, max_over_ranks, "bf16")
        if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"], line["parity"] = cpu_baseline_and_parity(blob, spec, rays_np, hip_outputs)
            line["parity"]["trained_like_weights"] = trained_like_parity(model, cfg, dev, spec, sorted(hip_outputs))
            line["parity"]["trained_long_weights"] = trained_like_parity(model, cfg, dev, spec, sorted(hip_outputs),
                                                                         "trained_llff_blob.npz" if spec["family"] == "llff" else "trained_long_blob.npz")
            if args.config == "C2":
                line["cpu_baseline_torch"] = torch_cpu_baseline(spec)
        if args.full and rank == 0 and world == 1 and args.config == "C2" and not args.no_other_configs:
            line["other_configs"] = other_configs(args, dev, sync, max_over_ranks)     # (re-parses the gin config: last)
    else:
        res = train_step_bench(args, spec, model, cfg, rays, rank, world, dev, dist, sync, max_over_ranks,
                               args.train_precision, n_steps=args.steps, n_warm=args.warmup, geometry=True)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, train_outputs(model, res["loss"]), rays_per_rank)
        line["dtype"] = args.train_precision
        if args.full and not args.no_train:
            # the other chain modes beside the headline step: exact fp32 chains (strict parity) and the bf16 throughput mode
            # (its gradient is 1e-1 relative L2 from the reference on trained-like weights)
            for other in [m for m in ("f32", "f16x2", "bf16") if m != args.train_precision]:
                line["train_step_" + other] = train_step_bench(args, spec, model, cfg, rays, rank, world, dev, dist, sync, max_over_ranks,
                                                               other, n_steps=max(2, args.steps // 4), n_warm=1, geometry=True)
        line["metric"] = (f"ray-samples/s ({spec['rays']} rays x {N} samples x 2 levels, Ref-NeRF LLFF geometry losses, "
                          "training step fwd+bwd+all-reduce+Adam)")
        line["value"] = res["value"]
        line["ms_per_step"] = res["ms_per_step"]
        line["roofline"] = res.pop("roofline")
        line["train_step"] = res
        if rccl is not None:
            line["rccl"] = rccl
        if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline_train(model, cfg, blob, spec, rays_np, rank)
    if rank == 0 and args.full:
        emit(line)
    elif rank == 0:
        emit_line(line)
    if dist is not None:
        dist.barrier()
    import torch.distributed as _d
    if _d.is_initialized():
        _d.destroy_process_group()


def train_step_bench(args, spec, model, cfg, rays, rank, world, dev, dist, sync, max_over_ranks, chains="f32",
                     n_steps=None, n_warm=1, geometry=False):
    """One full training step on the batch: training forward (density-gradient normals + saved layer inputs),
    losses (the three Ref-NeRF terms, or with `geometry` the nine-term set of llff_refnerf_geometry_losses.gin incl.
    the noisy-ray second pass), HIP backward + weight-gradient GEMM, ONE all-reduce of the gradient blob over the
    ranks, Adam step.  `chains` = arithmetic of the MLP chains of the training kernels ('f32' strict parity | 'f16x2' split-f16,
    the mode of record | 'bf16' throughput); the weight-gradient GEMM runs on split-bf16 MFMA at fp32 accuracy (f32 / bf16
    chains) or on f16 MFMA over the split-f16 formats (f16x2 chains)."""
    import torch
    from refnerf_pl_amd import _hip, distributed, synthetic, train_utils, utils
    model.train()
    fwd_chains = bwd_chains = chains                      # 'f32' | 'f16x2' (split-f16 chains both ways: parity-grade) | 'bf16'
    if os.environ.get("REFNERF_BENCH_BWD"):               # A/B: e.g. the f32 forward with the split-f16 backward (fp32 rows)
        bwd_chains = os.environ["REFNERF_BENCH_BWD"]
    cfg.hip_train_precision, cfg.hip_bwd_precision = fwd_chains, bwd_chains
    cfg.hip_fused_losses = True          # data + orientation + predicted-normal terms through the fused loss kernels
    cfg.hip_flat_grads = True            # gradient, all-reduce and Adam on ONE flat tensor per MLP
    R = rays.origins.shape[0]
    N = spec["samples"]
    gt = torch.as_tensor(synthetic.target_rgb(R, seed=7 + rank), device=dev)     # resident like the rays: no per-step H2D copy
    batch = utils.Batch(rays=rays, rgb=gt)
    mlps = list({id(x): x for x in (model.nerf_mlp, model.prop_mlp)}.values())
    opt = torch.optim.Adam([m.flat_parameter() for m in mlps], lr=1e-4, fused=True)
    extra_rays = cfg.sample_noise_size * cfg.sample_noise_angles if geometry else 0
    it = [0]

    def step():
        opt.zero_grad(set_to_none=True)
        if geometry:
            total, _, _, _ = train_utils.training_losses(model, batch, rays, cfg, global_step=200000 + it[0])
        else:
            renderings, history = model(rays, 1.0, False)
            total, _, _ = train_utils.compute_losses(model, batch, rays, renderings, history, cfg)
        total.backward()
        distributed.allreduce_gradients(model, force=dist is not None)      # (one-rank RCCL group of the single-GPU legs: still issued)
        opt.step()
        for m in mlps:
            m.mark_updated()               # fused Adam leaves no trace in the version counters: tell the weight-image cache
        it[0] += 1
        return total

    n = n_steps if n_steps is not None else max(2, min(10, args.steps // 3))
    for _ in range(max(1, n_warm)):
        step()
    sync()
    _hip.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(n):
        loss = step()
    sync()
    el = max_over_ranks(time.perf_counter() - t0)
    fam = {k: _hip.get_timing(f) for k, f in (("fwd", _hip.TIMER_FORWARD), ("bwd", _hip.TIMER_BACKWARD), ("wgrad", _hip.TIMER_WGRAD))}
    _hip.set_timing(False)
    model.eval()
    cfg.hip_train_precision = cfg.hip_bwd_precision = "f32"
    cfg.hip_flat_grads = cfg.hip_fused_losses = False
    assert os.environ.get("REFNERF_BENCH_PROBE") or torch.isfinite(loss.detach()).all()   # (timing probes of deliberately wrong builds set the env)
    rate = world * (R + extra_rays) * N * 2 * n / el
    # per-kernel rooflines from the event pairs of the timed steps (a level = one launch of each family; the noisy
    # pass of the geometry config launches the same kernels on fewer rays: averages are per launch over both)
    passes = 2 if geometry else 1           # clean + noisy pass: two launches of each family per level and step
    samples_per_launch = (R + extra_rays) * N / passes
    kernels = {}
    sq = fwd_chains == "f16x2" and bwd_chains == "f16x2" and not _hip.LEGACY_F16X2_TRAIN      # the round-5 kernels (eval skeleton)
    half_act = getattr(cfg, "hip_wgrad_mode", "bf16x3") == "f16"      # the forward that does not write the lo units of the spatial layer inputs
    names = {"fwd": ("rn::level_fwd_train_sq_h" if half_act else "rn::level_fwd_train_sq") if sq else "rn::level_fwd_train_" + {"bf16": "bf16c", "f16x2": "f16x2c", "f32": "f32"}[fwd_chains],
             "bwd": "rn::level_bwd_sq" if sq else "rn::level_bwd_" + {"bf16": "bf16c", "f16x2": "f16x2c", "f32": "f32"}[bwd_chains],
             "wgrad": "rn::wgrad_sq256_kernel" if sq else ("rn::wgrad_f16s_kernel" if (fwd_chains == "f16x2" and bwd_chains == "f16x2") else "rn::wgrad_bf16x3_kernel")}
    peak_of = {"fwd": PEAK_TFLOPS[fwd_chains], "bwd": PEAK_TFLOPS[bwd_chains]}
    for k, (ms, cnt) in fam.items():
        if not cnt:
            continue
        avg = ms / cnt
        if k == "wgrad":
            # algorithmic bytes: both operand matrices read once -- ACT (4396 rows) + DELTA (4244 rows) per sample,
            # fp32 rows in the f32 mode, bf16 rows with the bf16 chains
            # (split-f16 formats, round 4: ACT hi / lo pair units = 4 B per element, DELTA one half per element + 18 factor words)
            # (round 5, REFNERF_ACT_SQ: spatial ACT rows hi + lo = 4 B per element, directional ACT rows ONE half, DELTA one half
            #  + two factor words per layer: (96 + 2048) * 4 + (204 + 2048) * 2 + 4244 * 2 + 36 * 4 = 21.7 KB per ray-sample)
            act_sp = 2 if getattr(cfg, "hip_wgrad_mode", "bf16x3") == "f16" else 4       # 'f16': the spatial layer inputs at one half as well
            bytes_per_launch = samples_per_launch * (((96 + 2048) * act_sp + (204 + 2048) * 2 + 4244 * 2 + 36 * 4) if sq
                                                     else (4396 * 4 + 4244 * 2 + 18 * 4) if (fwd_chains == "f16x2" and bwd_chains == "f16x2")
                                                     else (4396 + 4244) * (2 if chains == "bf16" else 4))
            ach = bytes_per_launch / (avg * 1e-3) / 1e9
            tr, tsrc = traffic_of(names[k], spec.get("name", "C2"), R, N) if not geometry else (None, None)
            kernels[k] = {"kernel": names[k], "bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                          "frac": ach / PEAK_HBM_GBS, "avg_launch_ms": avg, "launches": cnt, "bytes_per_launch": bytes_per_launch,
                          "traffic": tr, "traffic_source": tsrc}
        else:
            # forward: MLP + density-normal VJP; backward kernel: the transposed chains dX = W^T delta (one pass over
            # the MLP's contractions -- the other half of the backward FLOPs, dW, is the wgrad GEMM's)
            flop = samples_per_launch * ((FLOP_PER_SAMPLE + NORMALS_VJP_FLOP) if k == "fwd" else FLOP_PER_SAMPLE)
            ach = flop / (avg * 1e-3) / 1e12
            tr, tsrc = traffic_of(names[k], spec.get("name", "C2"), R, N) if not geometry else (None, None)
            kernels[k] = dict({"kernel": names[k], "bound": "mfma", "achieved": ach, "peak": peak_of[k], "unit": "TFLOP/s",
                               "frac": ach / peak_of[k], "avg_launch_ms": avg, "launches": cnt, "flop_per_launch": flop,
                               "traffic": tr, "traffic_source": tsrc},
                              **({} if geometry else pmc_of(names[k], spec.get("name", "C2"), R, N)))
    out = {"value": rate, "unit": "ray-samples/s (fwd+bwd+Adam)", "ms_per_step": 1e3 * el / n, "steps": n,
           "dtype": chains, "wgrad": getattr(cfg, "hip_wgrad_mode", "bf16x3"), "losses": "fused kernels (Config.hip_fused_losses)", "gradients": "one flat tensor per MLP (Config.hip_flat_grads)",
           "loss": float(loss.detach()),
           "kernels": kernels,
           "kernels_ms_per_step": sum(ms for ms, _ in fam.values()) / n,
           "mode": ("parity mode: f32 MLP chains (gradient rel-L2 <= 2e-4 vs the reference's autograd, 1e-3 on trained-like weights)"
                    if chains == "f32" else
                    "parity-grade fast mode: forward and backward chains on split-f16 operands (22-bit products); ACT saved as hi / lo pair "
                    "units, DELTA as one half per element + a per-sample factor, weight gradients on f16 MFMA; gradient rel-L2 5e-5 .. 1.1e-4 vs "
                    "the reference's autograd, also on trained-like weights"
                    if chains == "f16x2" else
                    "throughput mode: bf16 MLP chains; gradient 1e-2 (random-init) / 1e-1 (trained-like weights) relative L2 from the "
                    "reference -- for from-scratch training, not a parity mode"),
           "note": "`kernels` holds one roofline per kernel family from HIP event pairs (chains against the MFMA peak of their "
                   "operand type, the weight-gradient GEMM against HBM); kernels_ms_per_step = their sum, the rest of ms_per_step "
                   "is losses, all-reduce, optimiser and weight re-pack"}
    if "fwd" in kernels:
        out["roofline"] = dict(kernels["fwd"], timing="HIP event pairs on the launch stream, inside the timed region")
    return out


if __name__ == "__main__":
    main()
