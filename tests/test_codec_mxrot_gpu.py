"""Rotated MX rows on the MXR kernels (csrc/codec.hip): the GPU's message and decode are the CPU oracle's bit for bit."""
from functools import lru_cache

import pytest
import torch

import test_codec_mxrot as M
from llm_inference_in_distributed_edge_networks_amd import codec as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
B, S, RATIO = 2, 5, 0.4
SHAPES = [32, 544, 2080]            # one block, one quad, NCH 1; 17 blocks, a partial chunk; 65 blocks: NCH 8, 2 FP6 passes
IMP = torch.tensor([[1, 3, 2, 8, 2], [4, 1, 1, 2, 8]]) / 16.0     # dyadic: the top-rho cut is the same in any order
CASES = [(n, e, "ratio") for n in M.MX_CODECS for e in (("fp4", "e2m3", "e3m2") if n != "mxfp8" else ("fp4",))] + \
    [("mixed_mxfp4_mxfp8", "fp4", "top_rho")]


@lru_cache(maxsize=None)
def rows(H, dtype):      # [10, H]: the CPU file's constructed rows, then randn with one x100 channel
    x = torch.randn(B * S, H, generator=torch.Generator().manual_seed(H))
    x[:, H // 2 + 3] *= 100
    x[:6] = M.unit_rows(H)
    return x.to(dtype)


def bits(t): return t.view(torch.int16 if t.dtype == BF16 else torch.int32)   # noqa: E704


@pytest.mark.parametrize("H", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,elem,sel", CASES)
def test_gpu_equals_cpu(name, elem, sel, dtype, H):
    spec = C.with_mx_rot(C.with_mx_elem(C.get_codec(name), elem), "h32")
    x = rows(H, dtype)
    finite = x.clone()
    finite[2:5, :32] = 0                                     # without the NaN, Inf and overflow blocks: every byte
    m_cpu, L = C.encode(finite, spec, B, S, RATIO, IMP, selection=sel)
    m_gpu, L2 = C.encode(finite.to(DEV), spec, B, S, RATIO, IMP.to(DEV), selection=sel)
    assert L2 == L and torch.equal(m_gpu.cpu(), m_cpu), f"{(m_gpu.cpu() != m_cpu).sum().item()} bytes differ"
    assert torch.equal(bits(C.decode(m_gpu, spec, L, dtype).cpu()), bits(C.decode(m_cpu, spec, L, dtype)))
    y_cpu = C.decode(C.encode(x, spec, B, S, RATIO, IMP, selection=sel)[0], spec, L, dtype)
    y = C.decode(C.encode(x.to(DEV), spec, B, S, RATIO, IMP.to(DEV), selection=sel)[0], spec, L, dtype).cpu()
    ok = y_cpu.isfinite()                                    # with them: non-finite on both sides, the rest bit for bit
    assert torch.equal(y.isfinite(), ok) and torch.equal(bits(y)[ok], bits(y_cpu)[ok])
    assert not ok[2, :32].any()                              # row 2 is an MX row in every case: its NaN block is 32 NaNs


def test_pipeline_boundary_equals_cpu_decode():
    """Stage 1's input on the GPU is the CPU pipeline's decode of the same rotated mixed MXFP4 / MXFP8 message (fp32)."""
    from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
    from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
    from llm_inference_in_distributed_edge_networks_amd.models import TINY_QWEN2 as cfg, DecoderLM
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan
    plan, bcfg = PipelinePlan.from_split_layers(cfg.num_layers, [1]), BoundaryConfig("mixed_mxfp4_mxfp8", 0.5, mx_rot="h32")
    gpu, cpu = (LocalPipeline(DecoderLM.random_init(cfg, 1, std=0.05, device=torch.device(d), dtype=F32), plan, bcfg)
                for d in (DEV, "cpu"))
    b = next(batches(synthetic_stream(1000, cfg.vocab_size, 3), sliding_windows(1000, 200, 32), 3))
    with torch.no_grad():
        x0, imp, _ = gpu.stages[0].run(b.to(DEV))
        msg, L = gpu.stages[0].encode(x0, b.to(DEV), imp)
        got = C.decode(msg, gpu.stages[1].spec_in, gpu.stages[1].layout_in(b.to(DEV)), F32)
        want = C.decode(msg.cpu(), cpu.stages[1].spec_in, cpu.stages[1].layout_in(b), F32)
        assert torch.isfinite(gpu.run_batch(b.to(DEV))).all()
    assert L.hi_fmt == C.wire.FMT_MXFP8R and L.lo_fmt == C.wire.FMT_MXFP4R and 0 < L.k < L.S
    assert torch.equal(bits(got.cpu()), bits(want)) and want.isfinite().all()
