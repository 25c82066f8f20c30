#!/usr/bin/env python
"""Headline benchmark: Qwen2-0.5B layer-wise split inference with an importance-quantized boundary, fp32.

Metric (BASELINE.json): "WikiText-2 PPL + inter-stage bytes/token, Qwen2-0.5B 2-stage split; tokens/sec".  One
step = ``--microbatches`` window batches of ``--batch`` windows (max_length 512, stride 32: the reference recipe,
``Experiments/Qwen2-0.5B/params.json``) per data-parallel replica, pushed through the stage pipeline:

    stage 0: embed -> layers 0..L (importance at L) -> boundary codec encode -> RCCL send
    stage s: RCCL recv -> decode -> its layers (importance at its last layer) -> encode -> send
    last   : recv -> decode -> its layers -> final norm + LM head + CE on the scored rows

N GPUs -> pp stages x dp = N/pp replicas, one process per GPU (``--pp`` 2 by default: the reference's two-device
split after layer ``--split``; ``--pp 4`` / ``--pp 8`` are BASELINE configs 4-5, cost-balanced stages).  N = 1 runs
the same stages in one process on the one GPU (the boundary is still encoded and decoded).

Launch: under ``torch.distributed.run`` the ranks come from the env (``--gpus`` must equal WORLD_SIZE, or the run
stops).  ``python bench.py --gpus N`` with N > 1 and no launcher env starts the N ranks itself: this process runs
``torch.distributed.run --nproc-per-node N`` as a child before it makes any GPU call, and exits with its code.  The
JSON line records the world size, the process-group backend and every rank's device.

Precision: ``--dtype fp32`` (default) is the reference's precision (it loads its models without a torch_dtype,
``Experiments/Qwen2-0.5B/qwen_layer_wise.py:17``): fp32 residual stream, norms, softmax, attention (split-bf16
matrix-core products) and codec, GEMMs on h3 split-fp16 operands (fp32-accurate, see ``ops.reference.h3_act``).
The random weights have bf16 VALUES held in fp32 tensors by default (``--weight-values``): that is what the reference
computes with, since the HF Qwen2-0.5B checkpoint stores bf16 (``torch_dtype: bfloat16``) and the reference upcasts
it to fp32.  Such weights are exact in fp16 after scaling, so their h3 GEMMs need two fp16 products instead of three
(the third is exactly zero).

A plain run does only what the headline needs: it sets up, warms up, times ``--steps`` steps, writes its outputs if
``--dump-outputs DIR`` is given and prints the JSON line.  ``--full`` adds the separately timed measurements and
checks: the same fp32 run on full-fp32 random weight values (``value_fp32_weights``, ``--no-fp32-weights`` skips it),
the bf16 mode (``value_bf16``, ``--no-bf16``), at N = 1 the reference's notebook sweep and the HF-eager reference path
on the same GPU, the box calibration, and at N > 1 the p2p probe of every pipeline edge, the N-stage pipeline
(``value_ppN``) and the per-transport check.

``--dump-outputs DIR`` writes what the timed path returned in its last timed step: ``DIR/window_nll.npy``, the
per-window NLL ``[micro-batch, window]`` of every ``run_batch`` call of that step (float32 or float64, as the
pipeline returned it).  Across GPUs (pp > 1 over ranks) the timed region is one continuous pipeline, whose caller
receives the accumulated NLL: every last-stage rank writes ``DIR/nll_sum.rank<r>.npy`` = [total NLL, scored tokens].
The token stream and the weights are seeded (``--seed``), so equal arguments give equal inputs from run to run.

``value`` = window tokens processed per second over the whole job (every window is a full 512-token forward, as in
the reference, except that the model's last layer, which feeds only the LM head, runs its O-projection / MLP on the
scored rows: identical NLL, ``config.last_layer_rows``); scored tokens/s, PPL and the wire bytes/token measured by the
senders' byte counters are reported alongside, plus a per-stage GPU time breakdown for pipelines across GPUs.  At
N > 1 with ``--full`` the headline pp2 x dp(N/2) run is followed by one N-stage pipeline over all the GPUs
(``value_ppN``, BASELINE configs 4-5), reported beside it.  Data: synthetic token stream of the WikiText-2 test
length, random-init
weights of the exact Qwen2-0.5B architecture (no network / HF cache on the benchmark machines), so the PPL is that
of random weights (~vocab size) and measures plumbing, not quality.
"""
from __future__ import annotations

import argparse
import gc
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from llm_inference_in_distributed_edge_networks_amd import codec as C  # noqa: E402
from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream  # noqa: E402
from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows  # noqa: E402
from llm_inference_in_distributed_edge_networks_amd.models import build_model, get_config  # noqa: E402
from llm_inference_in_distributed_edge_networks_amd.parallel import (BoundaryConfig, DistributedPipeline,  # noqa: E402
                                                                      Grid, LocalPipeline, PipelinePlan,
                                                                      init_distributed)
from llm_inference_in_distributed_edge_networks_amd.parallel.dist import all_reduce_max_  # noqa: E402

METRIC = "WikiText-2 PPL + inter-stage bytes/token, Qwen2-0.5B 2-stage split; tokens/sec"
# Reference throughput on its own hardware: the Qwen2 sweep ran 1 eager + 100 split fp32 forwards of
# 512 tokens per window at 16.03-16.35 s/window on a T4 = ~3.2k forward tokens/s.
BASELINE_TOKENS_PER_S = 3200.0
T4_SWEEP_S_PER_WINDOW = 16.19   # the same notebook's sweep: 16.03-16.35 s per window
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", default="qwen2-0.5b")
    p.add_argument("--dtype", default="fp32", choices=sorted(DTYPES))
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements and checks (full-fp32 weight values, bf16 mode, notebook "
                        "sweep, HF-eager reference path, box calibration; N > 1: p2p probe, N-stage pipeline, "
                        "transports); the --no-* options below drop single ones of them")
    p.add_argument("--dump-outputs", default="", metavar="DIR",
                   help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy")
    p.add_argument("--no-bf16", action="store_true", help="--full: skip the secondary bf16-mode measurement")
    p.add_argument("--batch", type=int, default=64, help="windows per micro-batch")
    p.add_argument("--microbatches", type=int, default=0,
                   help="micro-batches per step per replica (default 4 x pipeline depth across GPUs: every GPU does "
                        "the work of 4 full-model micro-batches per step at any N, i.e. weak scaling)")
    p.add_argument("--max-length", type=int, default=512)
    p.add_argument("--stride", type=int, default=32)
    p.add_argument("--pp", type=int, default=2, help="pipeline stages (2: the reference's two-device split)")
    p.add_argument("--split", type=int, default=11, help="pp=2: last layer of stage 0 (reference layer_of_interest)")
    p.add_argument("--codec", default="mixed_int4_int8")
    p.add_argument("--ratio", type=float, default=0.5)
    p.add_argument("--method", default="regular_importance")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--transport", default="torch", choices=["torch", "rccl", "ipc"],
                   help="stage hand-off: torch.distributed p2p (RCCL), the native RCCL wrapper, or peer copies into "
                        "IPC-mapped receive slots (ipc)")
    p.add_argument("--no-graphs", action="store_true")
    p.add_argument("--weight-values", default="bf16", choices=["bf16", "fp32"],
                   help="precision of the random weight VALUES (held in fp32 in the fp32 mode): bf16 = as the HF "
                        "Qwen2-0.5B checkpoint the reference upcasts to fp32 (torch_dtype bfloat16); fp32 = full fp32 "
                        "random values (reported as value_fp32_weights)")
    p.add_argument("--no-fp32-weights", action="store_true", help="--full: skip the fp32-valued-weights measurement")
    p.add_argument("--no-sweep", action="store_true",
                   help="--full, N = 1: skip the timing of the reference's notebook sweep (notebook_sweep)")
    p.add_argument("--no-hf-compare", action="store_true",
                   help="--full: skip the same-node reference-path measurement (HF transformers + eager, N = 1 only)")
    p.add_argument("--no-deep-pp", action="store_true",
                   help="--full, N > 1: skip the secondary measurement of one N-stage pipeline over all the GPUs "
                        "(value_ppN)")
    p.add_argument("--deep-pp-timeout", type=float, default=300.0,
                   help="N > 1: seconds a secondary measurement (deep pipeline, transports) or the shutdown may go "
                        "without progress before it counts as hung")
    p.add_argument("--no-transports", action="store_true",
                   help="--full, N > 1: skip the short per-transport check (torch p2p / native RCCL / IPC peer copies)")
    p.add_argument("--json-out", default="")
    return p.parse_args()


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_gpu_count() -> int:
    """GPUs this process could use, counted without touching the HIP runtime (the launcher parent must not
    initialise it before it starts the ranks): GPU nodes of the KFD topology in sysfs (nodes with SIMDs), capped by
    HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES when set.  0 = unknown (the ranks check)."""
    n = 0
    root = "/sys/class/kfd/kfd/topology/nodes"
    try:
        for node in os.listdir(root):
            try:
                with open(os.path.join(root, node, "properties")) as f:
                    props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            except OSError:
                continue
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except OSError:
        n = 0
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            ids = [x for x in v.split(",") if x.strip() != ""]
            n = min(n, len(ids)) if n else len(ids)
    return n


def shared_gpu() -> bool:
    return os.environ.get("EDGE_SHARED_GPU", "0") not in ("", "0")


def launch_mode(a) -> str:
    """"torchrun" (rank env present), "self" (--gpus N > 1 without it: spawn the ranks) or "single".

    Called before any GPU call, and makes none itself: the visible-GPU check reads sysfs and the environment
    (``visible_gpu_count``); the ranks check their devices again after they start."""
    if "WORLD_SIZE" in os.environ and "RANK" in os.environ:
        world = int(os.environ["WORLD_SIZE"])
        if world != a.gpus:
            raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks; "
                             f"refusing to report a run of a different size")
        return "torchrun" if world > 1 else "single"
    if a.gpus < 1:
        raise SystemExit(f"bench.py: --gpus must be >= 1 (got {a.gpus})")
    if a.gpus == 1:
        return "single"
    ndev = visible_gpu_count()
    if 0 < ndev < a.gpus and not shared_gpu():
        raise SystemExit(f"bench.py: --gpus {a.gpus} but only {ndev} GPU(s) are visible")
    return "self"


def self_launch(a) -> int:
    """Run this script as ``a.gpus`` ranks under torch.distributed.run (one process per GPU, rendezvous on
    127.0.0.1) and return the launcher's exit code.  Rank 0 prints the JSON line."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, EDGE_BENCH_LAUNCH="self")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC (RCCL peer mappings on this host driver)
    return subprocess.call(cmd, env=env)


def rank_devices(env) -> list:
    """[{rank, local_rank, device, pci}] of every rank (collective)."""
    me = {"rank": env.rank, "local_rank": env.local_rank, "device": str(env.device)}
    if env.device.type == "cuda":
        pr = torch.cuda.get_device_properties(env.device)
        me["pci"] = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
        me["name"] = pr.gcnArchName
    if not env.is_dist:
        return [me]
    out = [None] * env.world_size
    torch.distributed.all_gather_object(out, me)
    return out


def build_stage_model(a, env, cfg, dtype, pp, grid, plan, values=None):
    """(model, provenance) of this rank: the whole model (one process) or its pipeline stage's layers."""
    if not (env.world_size > 1 and pp > 1):
        return build_model(cfg, env.device, dtype, seed=a.seed, values=values)
    _, stage = grid.coords(env.rank)
    return build_model(cfg, env.device, dtype, seed=a.seed, layers=plan.stage_layers(stage),
                       with_embed=(stage == 0), with_head=(stage == pp - 1), values=values)


def measure(a, env, cfg, dtype, pp, grid, plan, timed_steps, warmup, values=None, probe_sizes=(), built=None,
            dump_dir=""):
    """Build the model/pipeline for ``dtype`` (random weights with ``values`` precision; or use ``built`` =
    ``build_stage_model``'s result, kept alive for the caller) and time ``timed_steps`` steps after ``warmup``.
    ``dump_dir``: write the outputs of the last timed step there (``dump_outputs``).  Returns a dict."""
    dev = env.device
    world = env.world_size
    dist_pp = world > 1 and pp > 1
    bcfg = BoundaryConfig(a.codec, a.ratio, a.method)
    model, prov = built if built is not None else build_stage_model(a, env, cfg, dtype, pp, grid, plan, values)
    if not dist_pp:
        runner = LocalPipeline(model, plan, bcfg, use_graphs=not a.no_graphs)
    else:
        runner = DistributedPipeline(model, plan, bcfg, grid, env.rank, use_graphs=not a.no_graphs,
                                     transport=a.transport)
    probe = None
    if dist_pp and probe_sizes:
        # per pipeline edge, before the timed region: a 1 MiB and a boundary-sized message on the active transport
        # (a first multi-GPU run shows a p2p pathology here instead of only as recv_wait_ms)
        mine = runner.probe_p2p(probe_sizes)
        gathered = [None] * world
        torch.distributed.all_gather_object(gathered, mine)
        probe = sorted((r for g in gathered for r in g), key=lambda r: (r["stage"], r["edge"][0], r["bytes"]))

    # ---- data: synthetic stream of WikiText-2 test length, HF sliding windows, staged on device
    tokens = synthetic_stream(299_078, cfg.vocab_size, a.seed)
    wins = [w for w in sliding_windows(tokens.shape[1], a.max_length, a.stride) if w.length == a.max_length]
    need = a.batch * a.microbatches * grid.dp
    pool = [b.to(dev) for b in batches(tokens, wins[: need * 4], a.batch)]
    pool_w = [b.weights.to(dev) for b in pool]   # per-window loss weights, resident (no H2D copy per step)
    nll_acc = torch.zeros(2, dtype=torch.float64, device=dev)
    per_step = a.microbatches * grid.dp
    reports = []
    last_step = []   # --dump-outputs: the per-window NLL of every micro-batch of the last timed step

    def run_steps(first_step: int, nsteps: int, timing: bool = False):
        """pp across GPUs: one continuous pipeline over all nsteps*microbatches (stages stay busy across step
        boundaries; the only fill/drain is at the ends of the timed region).  Otherwise micro-batch by micro-batch
        through the local stages."""
        idx = [(first_step * per_step + i) % len(pool) for i in range(nsteps * per_step)]
        if not dist_pp:
            dump = [] if os.environ.get("EDGE_DUMP_NLL") else None
            for n, j in enumerate(idx):
                wn = runner.run_batch(pool[j])
                if dump_dir and timing and n >= len(idx) - per_step:
                    last_step.append(wn.detach().clone())   # the graph's output buffer is reused by the next call
                nll_acc[0] += (wn.double() * pool_w[j]).sum()   # device-side accumulation: no host sync
                nll_acc[1] += pool_w[j].sum()
                if dump is not None:
                    dump.append(wn.detach().double().clone())
            if dump:   # debug: per-micro-batch per-window NLL, named like DistributedPipeline's dumps
                n = run_steps.dumps = getattr(run_steps, "dumps", 0) + 1
                torch.save(torch.stack([d.cpu() for d in dump]), f"{os.environ['EDGE_DUMP_NLL']}.local.{n - 1}.pt")
        else:
            acc, rep = runner.evaluate([pool[j] for j in idx], timing=timing)
            nll_acc[0] += acc.total_nll
            nll_acc[1] += acc.n_tokens
            reports.append(rep)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()
        if env.is_dist:
            torch.distributed.barrier()
            if dev.type == "cuda":
                torch.cuda.synchronize()

    run_steps(0, warmup)
    sync()
    nll_acc.zero_()
    reports.clear()
    t0 = time.perf_counter()
    run_steps(warmup, timed_steps, timing=True)
    sync()
    dt = time.perf_counter() - t0
    if env.is_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        all_reduce_max_(t)
        dt = float(t.item())
    last = (not dist_pp) or grid.coords(env.rank)[1] == pp - 1
    ppl = math.exp(float(nll_acc[0]) / float(nll_acc[1])) if last and float(nll_acc[1]) > 0 else 0.0
    if env.is_dist:
        t = torch.tensor([ppl], dtype=torch.float64, device=dev)
        all_reduce_max_(t)
        ppl = float(t.item())
    stage_reports = None
    if dist_pp:
        gathered = [None] * world
        torch.distributed.all_gather_object(gathered, reports[-1] if reports else {})
        stage_reports = [dict(r, rank=i) for i, r in enumerate(gathered)]
        # measured wire bytes per token of every boundary: the senders' byte counters (warmup + timed region), summed
        # over the data-parallel replicas of each stage (exact for variable-k top-rho messages too)
        wires = []
        for s in range(pp - 1):
            rs = [r for r in stage_reports if r.get("stage") == s]
            b, t = sum(r.get("wire_bytes", 0.0) for r in rs), sum(r.get("wire_tokens", 0.0) for r in rs)
            wires.append(b / t if t else 0.0)
    else:
        wires = runner.wire_bytes_per_token()
    if dump_dir:
        dump_outputs(dump_dir, env, last, dist_pp, last_step, nll_acc)
    if dist_pp:
        runner.close()
    del runner, model, built
    gc.collect()
    if dev.type == "cuda":
        torch.cuda.empty_cache()
    return {"dt": dt, "ppl": ppl, "prov": prov, "stages": stage_reports, "p2p": probe, "wires": wires}


def dump_outputs(path, env, last, dist_pp, last_step, nll_acc, limit=64 << 20) -> None:
    """``--dump-outputs``: what the timed path handed its caller, as float32 / float64 ``.npy`` files under ``path``.
    One process: ``window_nll.npy`` [micro-batches of the last timed step, windows].  Pipeline across ranks: every
    last-stage rank's ``nll_sum.rank<r>.npy`` = [total NLL, scored tokens] of the timed region."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    if not dist_pp:
        out = torch.stack(last_step) if last_step else torch.zeros(0)
        out = out if out.dtype in (torch.float32, torch.float64) else out.float()
        arrays = {"window_nll": out.cpu().numpy()}
    elif last:
        arrays = {f"nll_sum.rank{env.rank}": nll_acc.detach().double().cpu().numpy()}
    else:
        arrays = {}
    assert sum(v.nbytes for v in arrays.values()) <= limit, "--dump-outputs: more than 64 MB of outputs"
    for name, v in arrays.items():
        np.save(os.path.join(path, name + ".npy"), v)


def notebook_sweep(a, env, cfg, dtype, values, windows: int = 64, batch: int = 32) -> dict:
    """The reference's own workload, timed on this GPU: the Qwen2 notebook sweep (``Notebooks/qwen2-0.5B_experiment.ipynb``
    cells 8-12, ``Experiments/Qwen2-0.5B/main.py:151-197``): per window 4 importance methods x boundary layers
    [22, 18, 3, 23, 11] x ratios [0, .25, .5, .75, 1] with the Q1 one-global-scale int4 quantizer, i.e. the 1 eager + 100
    split forwards the reference runs per window, here through ``SweepEngine`` (one shared prefix forward per window
    batch, the (method, ratio) variants forked at each boundary) in the bench's precision.  ``windows`` windows after one
    warmup batch (graph capture); the reference ran 16.03-16.35 s/window on a T4.  Never fails the
    bench: an error is recorded instead."""
    from llm_inference_in_distributed_edge_networks_amd.eval.sweep import SweepConfig, SweepEngine
    t_all = time.time()
    try:
        model, _ = build_model(cfg, env.device, dtype, seed=a.seed, values=values)
        layers = [22, 18, 3, 23, 11] if cfg.num_layers == 24 else sorted({1, cfg.num_layers - 2})
        hw = torch.full((cfg.num_layers, cfg.num_heads), 1.0 / cfg.num_heads)
        sc = SweepConfig(["regular_importance", "weighted_importance", "last_row", "aggregate_till"], layers,
                         [0, 0.25, 0.5, 0.75, 1], codec="ref_int4_global", head_weights=hw)
        toks = synthetic_stream(299_078, cfg.vocab_size, a.seed + 1)
        wins = [w for w in sliding_windows(toks.shape[1], a.max_length, a.stride) if w.length == a.max_length]
        bl = [b.to(env.device) for b in batches(toks, wins[: windows + 2 * batch], batch)]
        warm = SweepEngine(model, sc)
        for b in bl[:2]:              # warmup: an eager prefix, then its HIP-graph capture
            warm.run_batch(b)
        if env.device.type == "cuda":
            torch.cuda.synchronize()
        passes = []
        for _ in range(3):            # three timed passes over the same windows (a single ~1 s pass varied 17 %)
            eng = SweepEngine(model, sc)  # fresh accumulators, the captured prefix graph kept
            eng._graphs = warm._graphs
            t0 = time.perf_counter()
            for b in bl[2:]:
                eng.run_batch(b)
            ppl = eng.ppl()           # host sync: every window's 100 configurations done
            if env.device.type == "cuda":
                torch.cuda.synchronize()
            passes.append(time.perf_counter() - t0)
        dt = sorted(passes)[1]        # the median pass
        n = eng.windows_done
        out = {"what": f"notebook sweep: 4 methods x layers {layers} x ratios [0,.25,.5,.75,1], ref_int4_global "
                       f"(Q1): {int(ppl.numel())} split configurations per window + the importance forward; median "
                       f"of 3 timed passes",
               "windows": n, "seconds": round(dt, 3), "pass_seconds": [round(x, 3) for x in passes],
               "windows_per_s": round(n / dt, 2),
               "s_per_window": round(dt / n, 5), "configs_per_window": int(ppl.numel()),
               "ppl_ratio0_random_weights": float(ppl.reshape(-1)[0]), "wall_s_incl_build": None}
        del eng, warm, model, bl
    except Exception as e:   # the headline stands without it
        out = {"error": f"{type(e).__name__}: {e}"[:300]}
    gc.collect()
    if env.device.type == "cuda":
        torch.cuda.empty_cache()
    out["wall_s_incl_build"] = round(time.time() - t_all, 2)
    return out


def same_node_reference(a, cfg, dev) -> dict:
    """The reference's own computation (HF transformers + PyTorch eager, fp32: importance forward with attention maps,
    then the layer-wise split forward with the boundary quantized) timed on this GPU right after our run, one window
    per call as the reference loops and 64 windows batched.  Never fails the bench: an error is recorded instead."""
    try:
        from llm_inference_in_distributed_edge_networks_amd.eval.hf_reference import ReferencePath
        ref = ReferencePath(cfg, dev, seed=a.seed)
        out = {"what": "reference computation on HF transformers + PyTorch eager, fp32, same GPU, same windows",
               "layer": a.split, "ratio": a.ratio,
               "batch1": ref.throughput(batch=1, windows=16, warmup=2, layer=a.split, ratio=a.ratio,
                                        max_length=a.max_length, stride=a.stride, seed=a.seed),
               "batch64": ref.throughput(batch=64, windows=128, warmup=1, layer=a.split, ratio=a.ratio,
                                         max_length=a.max_length, stride=a.stride, seed=a.seed)}
        ref.close()
    except Exception as e:   # transformers missing or an HF API change: the headline stands without it
        out = {"error": f"{type(e).__name__}: {e}"[:300]}
    gc.collect()
    if dev.type == "cuda":
        torch.cuda.empty_cache()
    return out


def box_calibration(dev) -> dict:
    """Box-speed reference measured right after the framework's runs, so that numbers from different boxes can be
    compared through the driver's own record (box to box the headline spans ~7 % at equal code): the sustained
    throughput of a plain library GEMM (hipBLASLt fp16, 8192^3, 40 back-to-back calls: long enough to settle at the
    chip's power-limited clock, as the bench's GEMMs do) and of a 1 GiB device copy (HBM).  Never fails the bench."""
    if dev.type != "cuda":
        return {"skipped": "cpu"}
    try:
        n = 8192
        a = torch.randn(n, n, device=dev, dtype=torch.float16)
        b = torch.randn(n, n, device=dev, dtype=torch.float16)
        c = torch.empty(n, n, device=dev, dtype=torch.float16)
        for _ in range(10):
            torch.matmul(a, b, out=c)
        torch.cuda.synchronize()
        reps = 40
        t0 = time.perf_counter()
        for _ in range(reps):
            torch.matmul(a, b, out=c)
        torch.cuda.synchronize()
        tf = 2.0 * n ** 3 * reps / (time.perf_counter() - t0) / 1e12
        del a, b, c
        src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            dst.copy_(src)
        torch.cuda.synchronize()
        bw = 2.0 * src.numel() * 10 / (time.perf_counter() - t0) / 1e9   # read + write
        del src, dst
        torch.cuda.empty_cache()
        return {"what": "same-box reference: hipBLASLt fp16 8192^3 GEMM (40 back-to-back) and a 1 GiB device copy",
                "hipblaslt_fp16_tflops": round(tf, 1), "hbm_copy_GBps": round(bw, 1)}
    except Exception as e:   # the headline stands without it
        return {"error": f"{type(e).__name__}: {e}"[:300]}


def main():
    a = parse()
    mode = launch_mode(a)
    if mode == "self":
        sys.exit(self_launch(a))
    env = init_distributed("auto")
    devices = rank_devices(env)
    cfg = get_config(a.model)
    world = env.world_size
    pp = a.pp
    if world > 1 and (pp > world or world % pp):
        raise SystemExit(f"--pp {pp} must divide the number of GPUs ({world})")
    dist_pp = world > 1 and pp > 1
    grid = Grid(world, pp if dist_pp else 1)
    if a.microbatches <= 0:
        a.microbatches = 4 * (pp if dist_pp else 1)
    plan = (PipelinePlan.from_split_layers(cfg.num_layers, [a.split]) if pp == 2 else
            PipelinePlan.balanced(cfg, pp, a.max_length, a.stride / a.max_length))
    dtype = DTYPES[a.dtype] if env.device.type == "cuda" else torch.float32

    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
    if env.device.type == "cuda" and torch.cuda.device_count() < (1 if shared_gpu() else local_world):
        raise SystemExit(f"bench.py: rank {env.rank} sees {torch.cuda.device_count()} GPU(s), "
                         f"needs {local_world} (one per local rank)")
    values = torch.bfloat16 if a.weight_values == "bf16" else None
    spec = C.get_codec(a.codec)
    msg_bytes = C.message_bytes(spec, a.batch, a.max_length, cfg.hidden_size, a.ratio, dtype)
    main_run = measure(a, env, cfg, dtype, pp, grid, plan, a.steps, a.warmup, values,
                       probe_sizes=(1 << 20, int(msg_bytes)) if a.full else (), dump_dir=a.dump_outputs)
    dt = main_run["dt"]
    tok_per_step = grid.dp * a.microbatches * a.batch * a.max_length
    scored_per_step = grid.dp * a.microbatches * a.batch * a.stride
    value = tok_per_step * a.steps / dt
    wires = main_run["wires"]
    second = fp32w = None
    if a.full and values is not None and not a.no_fp32_weights and dtype == torch.float32 and env.device.type == "cuda":
        fp32w = measure(a, env, cfg, dtype, pp, grid, plan, a.steps, a.warmup, None)
    if a.full and not a.no_bf16 and dtype == torch.float32 and env.device.type == "cuda":
        second = measure(a, env, cfg, torch.bfloat16, pp, grid, plan, a.steps, a.warmup, values)
    sweep = None
    if a.full and world == 1 and not a.no_sweep:
        sweep = notebook_sweep(a, env, cfg, dtype, values)
    hf = None   # last, so that nothing of it can touch the framework's own measurements
    if a.full and world == 1 and not a.no_hf_compare and env.device.type == "cuda":
        hf = same_node_reference(a, cfg, env.device)
    calib = box_calibration(env.device) if a.full and env.is_main else None
    dname = {torch.float32: "fp32", torch.bfloat16: "bf16"}[dtype]
    out = {
        "metric": METRIC,
        "value": round(value, 1), "unit": "tokens/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(1000 * dt / a.steps, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": round(value / BASELINE_TOKENS_PER_S, 2), "dtype": dname,
        "data": "synthetic (WikiText-2-test-length Zipf token stream), random-init weights"
                + (" with bf16 values held in fp32 (as the HF Qwen2-0.5B checkpoint, torch_dtype bfloat16, that the "
                   "reference upcasts to fp32)" if values is not None else ""),
        "config": {"model": cfg.name, "global_batch": grid.dp * a.microbatches * a.batch, "seq_len": a.max_length,
                   "stride": a.stride, "parallelism": f"pp{pp}xdp{grid.dp}" if dist_pp else f"local-pp{pp}",
                   "stage_layers": [[r.start, r.stop - 1] for r in (plan.stage_layers(s) for s in range(pp))],
                   "codec": a.codec, "ratio": a.ratio, "importance": a.method,
                   "transport": a.transport if dist_pp else "local", "hip_graphs": not a.no_graphs,
                   "gemm_precision": "h3 split-fp16 (fp32-accurate)" if dname == "fp32" else "bf16",
                   # the model's last layer feeds only the LM head: its O-projection / MLP run on the scored rows
                   # (the NLL is identical); "all" under EDGE_LAST_LAYER_ALL_ROWS=1
                   "last_layer_rows": "all" if os.environ.get("EDGE_LAST_LAYER_ALL_ROWS", "0") not in ("", "0")
                   else "scored"},
        "baseline_note": "T4 fp32, 1 eager + 100 split forwards of 512 tokens per window in 16.2 s (BASELINE.md)",
        "scored_tokens_per_s": round(scored_per_step * a.steps / dt, 1),
        "wire_bytes_per_token": [round(w, 2) for w in wires],
        "wire_bits_per_element": [round(8 * w / cfg.hidden_size, 3) for w in wires],
        "wire_compression_vs_fp32_reference": [round(4 * cfg.hidden_size / w, 3) for w in wires],
        "ppl_random_weights": main_run["ppl"], "weights": main_run["prov"],
        "world_size": world, "backend": env.backend,
        "launch": os.environ.get("EDGE_BENCH_LAUNCH", mode), "rank_devices": devices,
    }
    if main_run["stages"]:
        out["stages"] = main_run["stages"]
    if main_run["p2p"] is not None:
        out["p2p"] = main_run["p2p"]
    if fp32w is not None:   # the same fp32 run on full-fp32 random weight values (three-product h3 GEMMs)
        out["value_fp32_weights"] = round(tok_per_step * a.steps / fp32w["dt"], 1)
        out["ms_per_step_fp32_weights"] = round(1000 * fp32w["dt"] / a.steps, 3)
        out["ppl_random_weights_fp32_weights"] = fp32w["ppl"]
    if second is not None:
        out["value_bf16"] = round(tok_per_step * a.steps / second["dt"], 1)
        out["ms_per_step_bf16"] = round(1000 * second["dt"] / a.steps, 3)
        out["ppl_random_weights_bf16"] = second["ppl"]
        if second["stages"]:
            out["stages_bf16"] = second["stages"]
    if sweep is not None:   # the reference's own workload (101 forwards per window), through the sweep engine
        out["notebook_sweep"] = sweep
        if "windows_per_s" in sweep:
            out["sweep_windows_per_s"] = sweep["windows_per_s"]
            out["sweep_s_per_window"] = sweep["s_per_window"]
            out["sweep_s_per_window_t4"] = T4_SWEEP_S_PER_WINDOW
            out["sweep_speedup_vs_t4"] = round(T4_SWEEP_S_PER_WINDOW / sweep["s_per_window"], 1)
    if calib is not None:
        out["box_calibration"] = calib
        if "hipblaslt_fp16_tflops" in calib:   # headline per sustained library TFLOP/s: comparable across boxes
            out["value_per_box_tflops"] = round(value / calib["hipblaslt_fp16_tflops"], 2)
    if hf is not None:
        out["same_node_reference_path"] = hf
        for k in ("batch1", "batch64"):
            if k in hf and hf[k]["window_tokens_per_s"] > 0:
                out[f"vs_same_node_reference_{k}"] = round(value / hf[k]["window_tokens_per_s"], 2)
    # test hook (tuning mode only, so a stray variable never changes a production run): this rank dies here
    fail = os.environ.get("EDGE_BENCH_FAIL_RANK") if tuning_mode() else None
    if fail is not None and int(fail) == env.rank:
        raise RuntimeError(f"EDGE_BENCH_FAIL_RANK: rank {env.rank} fails on purpose")
    if env.is_dist:
        # every rank finished its measurement: only then does rank 0 report (a failed rank means no JSON line,
        # and the launcher - or the self-launching parent - exits non-zero)
        torch.distributed.barrier()
    emit = Emitter(out, a.json_out if env.is_main else "", env.is_main)
    if not env.is_dist:
        emit()
        return
    # N > 1: secondary measurements and the shutdown run under one watchdog; a hang anywhere after this point still
    # prints the headline (with the hung measurement marked) and exits 70, an exception is recorded in its field
    guard = Guard(env, emit, a.deep_pp_timeout)
    if a.full and dist_pp and world != pp and not a.no_deep_pp:
        key = f"pp{world}"
        res = guard.run(key, lambda: deep_pipeline(a, env, cfg, dtype, values, spec))
        emit.out[f"value_{key}"] = res.pop("value") if res else None
        emit.out[key] = res if res else {"error": guard.last_error}
    if a.full and dist_pp and not a.no_transports:
        emit.out["transports"] = transports_check(a, env, cfg, dtype, values, spec, pp, grid, plan, guard)
    emit()
    guard.close()


def tuning_mode() -> bool:
    return os.environ.get("EDGE_TUNING", "0") not in ("", "0")


class Emitter:
    """Prints the one JSON line (rank 0) exactly once: normally at the end of the run, or from the watchdog of the
    secondary measurements when one of them hangs (the headline is never lost; the process then exits 70)."""

    def __init__(self, out: dict, path: str, main: bool):
        import threading
        self.out, self.path, self.main = out, path, main
        self._lock, self._done = threading.Lock(), False

    def __call__(self):
        with self._lock:
            if self._done or not self.main:
                self._done = True
                return
            self._done = True
            print(json.dumps(self.out), flush=True)
            if self.path:
                with open(self.path, "w") as f:
                    json.dump(self.out, f, indent=1)


class Guard:
    """Runs the secondary measurements of an N > 1 run (``run``) and the final shutdown (``close``) under ONE
    watchdog that stays armed until the process group is destroyed.

    * An exception on any rank is recorded, never raised: the ranks agree on the outcome through the store (one key
      per rank and measurement), not through a collective, so a rank that failed early can never pair its agreement
      with a collective that the others are still inside (``measure`` gathers stage reports).
    * A hang (a measurement or the shutdown still running ``timeout`` seconds after its last progress) prints the JSON
      line - the headline plus ``{"error": ...}`` in the hung measurement's field - and exits: 0 for a secondary
      measurement (every rank's watchdog fires, the headline is complete), 70 for the shutdown.  A rank that raised
      while its peers sit in a collective of the same measurement ends this way too: collectives cannot be
      cancelled, the watchdog bounds the wait."""

    def __init__(self, env, emit: Emitter, timeout: float):
        from llm_inference_in_distributed_edge_networks_amd.utils.watchdog import Watchdog
        self.env, self.emit, self.timeout = env, emit, timeout
        self.current: str | None = None
        self.last_error = ""
        self._n = 0
        self.wd = Watchdog(timeout, "bench-secondary", on_timeout=self._hang).start()

    def _hang(self):
        """Watchdog: the JSON line with the hung measurement marked, then exit - 0 when a secondary measurement hung
        (the headline is complete and valid, the failure is in the JSON), 70 when the shutdown did."""
        key = self.current or "shutdown"
        msg = f"still running after {self.timeout:.0f} s (rank {self.env.rank})"
        if key.startswith("pp"):
            self.emit.out[f"value_{key}"] = None
        if key.startswith("transports."):
            self.emit.out.setdefault("transports", {})[key.split(".", 1)[1]] = {"error": msg}
        else:
            self.emit.out[key] = {"error": msg}
        self.emit()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(70 if key == "shutdown" else 0)

    def agree(self, err: str | None) -> list:
        """Every rank's error (None = ok) for the current measurement, exchanged through the store."""
        store = torch.distributed.distributed_c10d._get_default_store()
        base = f"edge_bench/{self._n}/{self.current}"
        store.set(f"{base}/{self.env.rank}", json.dumps(err))
        return [json.loads(store.get(f"{base}/{r}")) for r in range(self.env.world_size)]

    def run(self, key: str, fn):
        """``fn()``'s result, or None (``last_error`` says why) if it failed on any rank."""
        self.current = key
        self._n += 1
        self.wd.beat()
        err = res = None
        try:
            _test_hook(key, self.env.rank)
            res = fn()
        except Exception as e:   # recorded; the headline stands
            err = f"{type(e).__name__}: {e}"[:300]
        self.wd.beat()
        errs = self.agree(err)
        self.current = None
        bad = [f"rank {i}: {e}" for i, e in enumerate(errs) if e]
        self.last_error = "; ".join(bad)[:600]
        gc.collect()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        return None if bad else res

    def close(self):
        self.wd.beat()
        self.current = "shutdown"
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
        self.wd.stop()


def _test_hook(key: str, rank: int) -> None:
    """Tuning-mode-only fault injection into a secondary measurement: EDGE_BENCH_FAIL_SECONDARY / _HANG_SECONDARY =
    "<key>:<rank>" (rank "*": every rank) makes that rank raise / block inside measurement <key> (tests of Guard's error
    and hang paths)."""
    if not tuning_mode():
        return
    for var, hang in (("EDGE_BENCH_FAIL_SECONDARY", False), ("EDGE_BENCH_HANG_SECONDARY", True)):
        v = os.environ.get(var, "")
        if v and v.rsplit(":", 1)[0] == key and v.rsplit(":", 1)[1] in ("*", str(rank)):
            if hang:
                time.sleep(3600)
            raise RuntimeError(f"{var}: rank {rank} fails {key} on purpose")


def deep_pipeline(a, env, cfg, dtype, values, spec) -> dict:
    """N > 1, after the headline: the same step as ONE N-stage pipeline over all the GPUs (BASELINE config 4 at N = 4,
    config 5's shape at N = 8: cost-balanced stages, every boundary quantized), on the same process group and
    transport.  Reported as ``value_pp{N}`` plus its stage breakdown and p2p probe in ``pp{N}``; the primary fields
    are unchanged.  Runs under ``Guard`` (errors recorded, hangs reported)."""
    world = env.world_size
    grid = Grid(world, world)
    plan = PipelinePlan.balanced(cfg, world, a.max_length, a.stride / a.max_length)
    steps, warm = max(2, a.steps // 2), max(1, a.warmup // 2)
    sub = argparse.Namespace(**vars(a))
    sub.microbatches = 4 * world          # weak scaling: every GPU does 4 full-model micro-batches per step
    t0 = time.time()
    msg_bytes = C.message_bytes(spec, a.batch, a.max_length, cfg.hidden_size, a.ratio, dtype)
    res = measure(sub, env, cfg, dtype, world, grid, plan, steps, warm, values, probe_sizes=(1 << 20, int(msg_bytes)))
    tok = sub.microbatches * a.batch * a.max_length   # dp = 1
    return {
        "value": round(tok * steps / res["dt"], 1),
        "parallelism": f"pp{world}xdp1", "steps": steps, "warmup": warm,
        "ms_per_step": round(1000 * res["dt"] / steps, 3), "global_batch": sub.microbatches * a.batch,
        "stage_layers": [[r.start, r.stop - 1] for r in (plan.stage_layers(s) for s in range(world))],
        "wire_bytes_per_token": [round(w, 2) for w in res["wires"]], "ppl_random_weights": res["ppl"],
        "stages": res["stages"], "p2p": res["p2p"], "wall_s": round(time.time() - t0, 2)}


TRANSPORTS = ("torch", "rccl", "ipc")


def transports_check(a, env, cfg, dtype, values, spec, pp, grid, plan, guard: Guard) -> dict:
    """N > 1: the native stage hand-offs on the real process layout.  One short pp step (the headline's
    grid and codec, ``--batch`` capped at 8 windows, 1 warmup + 1 timed step) per transport on ONE stage model: first
    torch.distributed p2p (the reference PPL), then the native RCCL wrapper (``RcclComm``: a 2-rank communicator per
    pipeline edge bootstrapped through the store) and the peer-copy transport (``IpcP2P``).  Per transport: the p2p
    probe rows of every edge, ``ms_per_step``, the PPL and whether it equals torch-p2p's (rel 1e-9: the same windows
    through the same graphs, so any difference is a transport bug).  A transport that fails (RCCL refuses ranks sharing
    a GPU) or hangs is recorded as ``{"error": ...}``."""
    t0 = time.time()
    sub = argparse.Namespace(**vars(a))
    sub.batch = min(a.batch, 8)
    sub.microbatches = 2 * pp
    msg_bytes = C.message_bytes(spec, sub.batch, a.max_length, cfg.hidden_size, a.ratio, dtype)
    out: dict = {"what": "one short pp step per stage hand-off (torch.distributed p2p = reference PPL); PPL must be "
                         "equal at rel 1e-9", "batch": sub.batch, "microbatches": sub.microbatches}
    built = guard.run("transports.model", lambda: build_stage_model(a, env, cfg, dtype, pp, grid, plan, values))
    if built is None:
        out["error"] = guard.last_error
        return out
    ref_ppl = None
    for t in TRANSPORTS:
        if t != "torch" and env.device.type != "cuda":
            out[t] = {"skipped": "CPU ranks: the native transports need GPUs"}
            continue
        if t == "rccl" and shared_gpu():
            # RCCL refuses ranks that share a device: ncclCommInitRank returns an error, or on some runs blocks until
            # the watchdog fires (the round-6 full-suite run stalled there); never attempted in the rehearsal
            out[t] = {"error": "not attempted: ncclCommInitRank refuses ranks sharing one GPU (EDGE_SHARED_GPU "
                               "rehearsal); the native RCCL channels need one GPU per rank"}
            continue
        sub_t = argparse.Namespace(**vars(sub))
        sub_t.transport = t
        r = guard.run(f"transports.{t}", lambda: measure(sub_t, env, cfg, dtype, pp, grid, plan, 1, 1, values,
                                                         probe_sizes=(1 << 20, int(msg_bytes)), built=built))
        if r is None:
            out[t] = {"error": guard.last_error}
            continue
        row = {"ms_per_step": round(1000 * r["dt"], 3), "ppl_random_weights": r["ppl"], "p2p": r["p2p"]}
        if t == "torch":
            ref_ppl = r["ppl"]
        elif ref_ppl:
            row["rel_diff_vs_torch"] = abs(r["ppl"] - ref_ppl) / ref_ppl
            row["ppl_equal_torch"] = row["rel_diff_vs_torch"] <= 1e-9
        out[t] = row
    del built
    out["wall_s"] = round(time.time() - t0, 2)
    return out


if __name__ == "__main__":
    main()
