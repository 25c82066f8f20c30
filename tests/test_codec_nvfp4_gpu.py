"""NVFP4 rows on the NV4 instantiations of pack_kernel / unpack_kernel (csrc/codec.hip nv_pack8 / nv_unpack8): the GPU's
message is the CPU oracle's byte for byte, its decode bit for bit.  B = 2, S = 5: 10 rows, so the last workgroup has idle
waves."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import test_codec_nvfp4 as N
from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
B, S = 2, 5
SHAPES = [32, 544, 896, 4096]       # two blocks, one quad; two blocks alone in chunk 1 (NCH 2); the model's; NCH 8
CASES = [(n, r) for n in N.MX_CODECS for r in ((0.0, 0.5, 1.0) if C.get_codec(n).uses_ratio else (0.0,))]


@lru_cache(maxsize=None)
def rows(H, dtype, nonfinite=False):
    """([10, H], importance): scale-byte and code tie / saturation rows, zero, zero-block, denormal, massive and Gaussian
    rows; ``nonfinite``: the NaN and the -Inf row in place of two of them (rows 4 and 5)."""
    g, u = torch.Generator().manual_seed(H), N.unit_rows(H)
    hard = [N.hard_row(N.scale_blocks(), 0, H), N.hard_row(N.scale_blocks(), -20, H, 255), N.hard_row(N.code_blocks(), 0, H),
            N.hard_row(N.code_blocks(), 100, H, 20)]
    x = torch.cat([torch.tensor(np.stack(hard)), u[[3, 4] if nonfinite else [0, 1]], u[[2, 5]], torch.randn(2, H, generator=g)])
    return x.to(dtype), torch.rand(B, S, generator=g)


def bits(t): return t.view(torch.int16 if t.dtype == BF16 else torch.int32)   # noqa: E704


@pytest.mark.parametrize("H", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,ratio", CASES)
def test_gpu_equals_cpu(name, ratio, dtype, H):
    spec = N.nv(name)
    x, imp = rows(H, dtype)
    m_cpu, L = C.encode(x, spec, B, S, ratio, imp)
    m_gpu, L2 = C.encode(x.to(DEV), spec, B, S, ratio, imp.to(DEV))
    assert L2 == L and W.FMT_NVFP4 in (L.hi_fmt, L.lo_fmt)
    assert torch.equal(m_gpu.cpu(), m_cpu), f"{(m_gpu.cpu() != m_cpu).sum().item()} bytes differ"
    assert torch.equal(bits(C.decode(m_gpu, spec, L, dtype).cpu()), bits(C.decode(m_cpu, spec, L, dtype)))


@pytest.mark.parametrize("H", SHAPES)
def test_nonfinite_rows_and_foreign_messages(H):
    """Only the code and scale bytes of the NaN and the -Inf row may differ from the CPU's; a foreign header decodes to NaN."""
    spec, rb = N.nv("mxfp4"), 9 * H // 16 + 4
    x, _ = rows(H, F32, True)
    m_cpu, L = C.encode(x, spec, B, S)
    m_dev, _ = C.encode(x.to(DEV), spec, B, S)
    m_gpu, free = m_dev.cpu(), torch.zeros(L.total, dtype=torch.bool)
    for r in (4, 5):                                         # the bytes that may differ: codes and scales, not g
        free[L.off_hi + r * rb:L.off_hi + (r + 1) * rb - 4] = True
    g_cpu, g_gpu = (N.fields(m[L.off_hi:L.off_hi + B * S * rb], H)[2] for m in (m_cpu, m_gpu))
    assert np.isnan(g_cpu[4]) and g_cpu[5] == np.inf and np.isfinite(g_cpu[[0, 1, 2, 3, 6, 7, 8, 9]]).all()
    assert np.array_equal(g_cpu.view(np.int32), g_gpu.view(np.int32)) and torch.equal(m_gpu[~free], m_cpu[~free])
    y, y_cpu = C.decode(m_dev, spec, L, F32).cpu(), C.decode(m_cpu, spec, L, F32)
    bad = torch.zeros(B * S, H, dtype=torch.bool)
    bad[4:6] = True
    assert torch.equal(y.isnan(), bad) and torch.equal(y_cpu.isnan(), bad) and torch.equal(bits(y)[~bad], bits(y_cpu)[~bad])
    m_dev[28:32] = 0
    m_dev[28] = W.FMT_MXFP4                                  # what the header of an unmodified mxfp4 message says
    assert bool(C.decode(m_dev, spec, L, F32).isnan().all())


def test_unsupported_combinations_are_rejected():
    """Format 26 beside head-group, 16-bit, 6-bit, rotated MX, outlier, h128 or row-rotated rows (formats 7 .. 25), in
    both class positions, on both entry points: hipErrorInvalidValue (1), and nothing is launched."""
    from llm_inference_in_distributed_edge_networks_amd.ops import _native
    H = 128
    L = C.layout(N.nv("mixed_mxfp4_mxfp8"), B, S, H, 2, F32)
    msg = torch.full((1 << 14,), 0xAB, dtype=torch.uint8, device=DEV)
    x = torch.full((B * S, H), 7.0, dtype=F32, device=DEV)
    for other in range(W.FMT_GRP, W.FMT_NVFP4):
        for hi, lo in ((W.FMT_NVFP4, other), (other, W.FMT_NVFP4)):
            for entry, x_f32 in (("edge_pack", 1), ("edge_pack", 0), ("edge_unpack", 1), ("edge_unpack", 0)):
                rc = getattr(_native.lib(), entry)(x.data_ptr(), msg.data_ptr(), L.off_mask, L.off_scale, L.off_hi, L.off_lo,
                                                   -1, 0, B, S, H, 2, hi, lo, W.SC_TOKEN, 127, 7, 0, 1024, x_f32,
                                                   _native.stream())
                assert rc == 1, (entry, hi, lo, rc)
    torch.cuda.synchronize()
    assert bool((msg == 0xAB).all()) and bool((x == 7.0).all())


def test_pipeline_in_a_captured_graph():
    """NVFP4 lo rows at a LocalPipeline boundary: graph replays equal eager, counted bytes are the modified layout's."""
    from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
    from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
    from llm_inference_in_distributed_edge_networks_amd.models import TINY_QWEN2 as cfg, DecoderLM
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan
    model = DecoderLM.random_init(cfg, 1, std=0.05, device=torch.device(DEV), dtype=F32)
    ids = synthetic_stream(1000, cfg.vocab_size, 3)
    bl = [b.to(DEV) for b in batches(ids, sliding_windows(1000, 200, 32), 5) if b.B == 5][:4]
    plan, bcfg = PipelinePlan.from_split_layers(cfg.num_layers, [1]), BoundaryConfig("mixed_mxfp4_mxfp8", 0.5, mx_elem="nvfp4")
    graph, eager = LocalPipeline(model, plan, bcfg), LocalPipeline(model, plan, bcfg, use_graphs=False)
    with torch.no_grad():
        for b in bl:                                         # eager, capture + replay, replay, replay
            assert torch.equal(graph.run_batch(b).clone(), eager.run_batch(b))
    assert len(bl) == 4 and graph.graphs.graphs, "nothing was captured"
    L = C.layout(bcfg.spec, 5, bl[0].S, cfg.hidden_size, W.num_lo(bcfg.spec, 0.5, bl[0].S), F32)
    assert L.lo_fmt == W.FMT_NVFP4 and graph.wire_bytes_per_token()[0] == L.total / (5 * bl[0].S)
