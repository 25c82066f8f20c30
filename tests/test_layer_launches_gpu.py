"""The model, the relevance engines, the pipeline and the sweep launch the recorded kernel sequences.

``tests/golden/layer_launches.json`` holds, per scenario, every call that reaches the kernel library through
``ops.call`` / ``codec.wire.call``: the entry-point name and its arguments, pointers reduced to null / non-null
(positions from ``_native._SIGS``), ints as they are, floats by ``repr``.  The Python layer that strings the kernels
together may be rearranged freely as long as every scenario's list stays equal to the fixture: the same kernels, in
the same order, on the same shapes, scales and optional operands.

Scenarios (the smallest shapes that reach every branch of ``DecoderLM.layer`` / ``layer_rows``):

* ``tiny-qwen2`` / ``tiny-neox`` x bf16 / fp32, B = 2, S = 40 (no multiple of 64: the padded V^T allocations):
  ``layer(0)`` without stats, with "lastrow" and with both statistics, ``layer_rows`` of the last layer at the last 3
  rows of each window;
* the fp32 fused RMSNorm-2 path: one Qwen2-0.5B-shaped layer at M = 32 * 512 = 16384 rows, the smallest M the
  256x224-tile kernel takes (64 row tiles x 4 column tiles = 256 CUs);
* both relevance engines with every optional table on both tiny models;
* a 2-stage eager ``LocalPipeline`` and a ``SweepEngine`` (eager prefix plus ``run_batch``) on one batch of two
  windows with different numbers of scored rows, with ``EDGE_LAST_LAYER_ALL_ROWS`` unset and set.

``python tests/test_layer_launches_gpu.py OUT.json`` records the fixture (on a GPU, from a commit whose launch
sequences are the wanted ones).
"""
import contextlib
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_inference_in_distributed_edge_networks_amd import ops
from llm_inference_in_distributed_edge_networks_amd.codec import wire
from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
from llm_inference_in_distributed_edge_networks_amd.eval.sweep import SweepConfig, SweepEngine
from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
from llm_inference_in_distributed_edge_networks_amd.models import QWEN2_0_5B, TINY_NEOX, TINY_QWEN2, DecoderLM
from llm_inference_in_distributed_edge_networks_amd.ops import _native
from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan
from llm_inference_in_distributed_edge_networks_amd.relevance.engine import RelevanceEngine
from llm_inference_in_distributed_edge_networks_amd.relevance.engine_f32 import RelevanceEngineH3

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_launches.json")
B, S = 2, 40
CFGS = {"tiny-qwen2": TINY_QWEN2, "tiny-neox": TINY_NEOX}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
ALL_ROWS = "EDGE_LAST_LAYER_ALL_ROWS"


@contextlib.contextmanager
def recorded():
    """Every ``ops.call`` / ``wire.call`` inside the block, as [name, arg, ...] rows (the calls still run)."""
    log = []

    def rec(name, *args):
        row = [name]
        for kind, a in zip(_native._SIGS[name], args):
            if kind is _native.c_p:
                row.append("ptr" if a else "null")
            elif kind is _native.c_f:
                row.append(repr(float(a)))
            else:
                row.append(int(a))
        assert len(row) == 1 + len(_native._SIGS[name]), name
        log.append(row)
        return _native.call(name, *args)

    saved = ops.call, wire.call
    ops.call = wire.call = rec
    try:
        yield log
    finally:
        ops.call, wire.call = saved


@contextlib.contextmanager
def all_rows_env(on: bool):
    old = os.environ.pop(ALL_ROWS, None)
    if on:
        os.environ[ALL_ROWS] = "1"
    try:
        yield
    finally:
        os.environ.pop(ALL_ROWS, None)
        if old is not None:
            os.environ[ALL_ROWS] = old


def _hidden(M, H, dtype):
    g = torch.Generator().manual_seed(1)
    return torch.randn(M, H, generator=g).to("cuda", dtype)


def layer_scenarios(model: str, mode: str) -> dict:
    cfg = CFGS[model]
    m = DecoderLM.random_init(cfg, 0, device="cuda", dtype=DTYPES[mode])
    x = _hidden(B * S, cfg.hidden_size, DTYPES[mode])
    rows = (torch.arange(B).view(-1, 1) * S + torch.arange(S - 3, S)).reshape(-1).cuda()
    n_rows = torch.full((B,), 3.0, device="cuda")
    out = {}
    for tag, stats in (("none", None), ("lastrow", "lastrow"), ("both", ("lastrow", "colsum"))):
        with recorded() as log:
            m.layer(0, x, B, S, stats=stats)
        out[f"{model}/{mode}/layer/{tag}"] = log
    with recorded() as log:
        m.layer_rows(cfg.num_layers - 1, x, B, S, rows, n_rows)
    out[f"{model}/{mode}/layer_rows"] = log
    return out


def fused_norm_f32_scenario() -> dict:
    cfg = QWEN2_0_5B.replace(num_layers=1, vocab_size=512)   # one Qwen2-0.5B-shaped layer; no embedding, no head
    m = DecoderLM.random_init(cfg, 0, device="cuda", dtype=torch.float32, layers=range(1), with_embed=False,
                              with_head=False)
    m.fuse_norm_f32 = True
    Bn, Sn = 32, 512
    assert m._np_fused(Bn * Sn) and not m._np_fused(Bn * Sn - 256)
    x = _hidden(Bn * Sn, cfg.hidden_size, torch.float32)
    with recorded() as log:
        m.layer(0, x, Bn, Sn)
    return {"qwen2-0.5b/fp32/fused-norm/layer": log}


def relevance_scenarios(model: str, mode: str) -> dict:
    cfg = CFGS[model]
    m = DecoderLM.random_init(cfg, 0, device="cuda", dtype=DTYPES[mode])
    eng = RelevanceEngineH3(m) if mode == "fp32" else RelevanceEngine(m)
    ids = torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(2))
    with recorded() as log:
        eng.head_relevance(ids, want_channels=True, want_sens=True, want_qerr=True)
    return {f"{model}/{mode}/relevance": log}


def _batch():
    """One batch of two windows: window 0 scores all its 39 rows, window 1 its last 8."""
    toks = synthetic_stream(200, TINY_QWEN2.vocab_size, 3)
    b = next(batches(toks, sliding_windows(200, S, 8), B)).to("cuda")
    assert b.n_rows.tolist() == [S - 1, 8]
    return b


def pipeline_scenarios(mode: str) -> dict:
    cfg = TINY_QWEN2
    m = DecoderLM.random_init(cfg, 0, device="cuda", dtype=DTYPES[mode])
    plan = PipelinePlan.from_split_layers(cfg.num_layers, [1])
    b = _batch()
    out = {}
    for on in (False, True):
        with all_rows_env(on):
            pipe = LocalPipeline(m, plan, BoundaryConfig("mixed_int4_int8", 0.5, "last_row"), use_graphs=False)
            with recorded() as log:
                pipe.run_batch(b)
        assert pipe.stages[-1].rows_only == (not on)
        out[f"pipeline/{mode}/{'all-rows' if on else 'scored-rows'}"] = log
    return out


def sweep_scenarios(mode: str) -> dict:
    """Boundary layers [1]: the prefix takes the scored-rows short cut; [3]: the last layer is a saved boundary, so
    the prefix runs it on every row whatever the switch says."""
    m = DecoderLM.random_init(TINY_QWEN2, 0, device="cuda", dtype=DTYPES[mode])
    b = _batch()
    out = {}
    for layers in ([1], [3]):
        for on in (False, True):
            with all_rows_env(on):
                sc = SweepConfig(["regular_importance", "last_row"], layers, [0, 0.5], codec="mixed_int4_int8")
                eng = SweepEngine(m, sc, use_graphs=False)
                with recorded() as log:
                    eng._prefix_eager(b)
                    eng.run_batch(b)
            out[f"sweep/{mode}/boundary{layers[0]}/{'all-rows' if on else 'scored-rows'}"] = log
    return out


GROUPS = {}
for _model in CFGS:
    for _mode in DTYPES:
        GROUPS[f"layer-{_model}-{_mode}"] = (layer_scenarios, (_model, _mode), f"{_model}/{_mode}/layer")
        GROUPS[f"relevance-{_model}-{_mode}"] = (relevance_scenarios, (_model, _mode), f"{_model}/{_mode}/relevance")
for _mode in DTYPES:
    GROUPS[f"pipeline-{_mode}"] = (pipeline_scenarios, (_mode,), f"pipeline/{_mode}/")
    GROUPS[f"sweep-{_mode}"] = (sweep_scenarios, (_mode,), f"sweep/{_mode}/")
GROUPS["fused-norm-f32"] = (fused_norm_f32_scenario, (), "qwen2-0.5b/fp32/fused-norm/")


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_launches_equal_fixture(group, fixture):
    fn, args, prefix = GROUPS[group]
    with torch.no_grad():
        got = fn(*args)
    torch.cuda.synchronize()
    assert set(got) == {k for k in fixture if k.startswith(prefix)}   # every recorded scenario is still run
    for name, log in got.items():
        want = fixture[name]
        assert log, name
        for n, (g, w) in enumerate(zip(log, want)):
            assert g == w, f"{name}: call {n} is {g}, recorded {w}"
        assert len(log) == len(want), f"{name}: {len(log)} calls, recorded {len(want)}"


if __name__ == "__main__":
    rec = {}
    with torch.no_grad():
        for key in sorted(GROUPS):
            fn, args, _ = GROUPS[key]
            rec.update(fn(*args))
    torch.cuda.synchronize()
    with open(sys.argv[1], "w") as f:
        f.write("{\n" + ",\n".join(
            json.dumps(k) + ": [\n" + ",\n".join("  " + json.dumps(r) for r in v) + "\n]"
            for k, v in sorted(rec.items())) + "\n}\n")
    print({k: len(v) for k, v in rec.items()})
