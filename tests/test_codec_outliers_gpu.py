"""Outlier rows on the OUT kernels (csrc/codec.hip): the GPU's message and decode are the CPU oracle's bit for bit."""
import pytest
import torch

import test_codec_outliers as O
from llm_inference_in_distributed_edge_networks_amd import codec as C

pytestmark = pytest.mark.gpu
DEV, F32, BF16 = "cuda", torch.float32, torch.bfloat16
B, S, RATIO, IMP = O.B, O.S, O.RATIO, O.IMP


def bits(t): return t.view(torch.int16 if t.dtype == BF16 else torch.int32)   # noqa: E704


@pytest.mark.parametrize("H", [32, 544, 2080])   # one lane group, NCH 1; a partial second chunk; NCH 8, outliers past 2048
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,sel", O.CASES)
def test_gpu_equals_cpu(name, sel, dtype, H):
    spec = C.with_outliers(C.get_codec(name), "top8")
    x = O.hard_rows(H).to(dtype)
    finite = x.clone()
    finite[6:9] = x[:3].flip(1)                              # without the NaN / Inf rows: every byte
    m_cpu, L = C.encode(finite, spec, B, S, RATIO, IMP, selection=sel)
    m_gpu, L2 = C.encode(finite.to(DEV), spec, B, S, RATIO, IMP.to(DEV), selection=sel)
    assert L2 == L and torch.equal(m_gpu.cpu(), m_cpu), f"{(m_gpu.cpu() != m_cpu).sum().item()} bytes differ"
    good = C.decode(m_cpu, spec, L, dtype)
    assert torch.equal(bits(C.decode(m_gpu, spec, L, dtype).cpu()), bits(good))
    y_cpu = C.decode(C.encode(x, spec, B, S, RATIO, IMP, selection=sel)[0], spec, L, dtype)
    y = C.decode(C.encode(x.to(DEV), spec, B, S, RATIO, IMP.to(DEV), selection=sel)[0], spec, L, dtype).cpu()
    ok = y_cpu.isfinite()                                    # with them: non-finite on both sides, the rest bit for bit
    assert torch.equal(y.isfinite(), ok) and torch.equal(bits(y)[ok], bits(y_cpu)[ok])
    m_gpu[(L.off_lo + L.row_bytes(L.lo_fmt) if L.k else L.off_hi + L.row_bytes(L.hi_fmt)) - 1] = 255   # a channel >= H
    bad = C.decode(m_gpu, spec, L, dtype).cpu()
    nan = bad.isnan().all(1)
    assert nan.sum() == 1 and torch.equal(bits(bad)[~nan], bits(good)[~nan])


def test_pipeline_boundary_equals_cpu_decode():   # stage 1's input on the GPU: the CPU decode of the same message
    from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
    from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
    from llm_inference_in_distributed_edge_networks_amd.models import TINY_QWEN2 as cfg, DecoderLM
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan
    plan, bcfg = PipelinePlan.from_split_layers(cfg.num_layers, [1]), BoundaryConfig("mixed_int4_int8", 0.5, outliers="top8")
    gpu, cpu = (LocalPipeline(DecoderLM.random_init(cfg, 1, std=0.05, device=torch.device(d), dtype=F32), plan, bcfg)
                for d in (DEV, "cpu"))
    b = next(batches(synthetic_stream(1000, cfg.vocab_size, 3), sliding_windows(1000, 200, 32), 3))
    with torch.no_grad():
        x0, imp, _ = gpu.stages[0].run(b.to(DEV))
        msg, L = gpu.stages[0].encode(x0, b.to(DEV), imp)
        got = C.decode(msg, gpu.stages[1].spec_in, gpu.stages[1].layout_in(b.to(DEV)), F32)
        want = C.decode(msg.cpu(), cpu.stages[1].spec_in, cpu.stages[1].layout_in(b), F32)
        assert torch.isfinite(gpu.run_batch(b.to(DEV))).all()
    assert L.hi_fmt == C.wire.FMT_INT8O and L.lo_fmt == C.wire.FMT_INT4O and 0 < L.k < L.S
    assert torch.equal(bits(got.cpu()), bits(want)) and want.isfinite().all()
