"""MXFP6 rows on the MX6 instantiations of pack_kernel / unpack_kernel (csrc/codec.hip): the GPU's message is the CPU
oracle's byte for byte, its decode bit for bit.  B = 2, S = 5: 10 rows, so the last workgroup has idle waves."""
from functools import lru_cache

import pytest
import torch

import test_codec_mx6 as M
from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
B, S = 2, 5
SHAPES = [32, 544, 896, 4096]       # one block, one lane; 17 blocks, one alone in chunk 1; 28 lanes, NCH 2; NCH 8, 2 passes
CASES = [(n, r) for n in M.MX_CODECS for r in ((0.0, 0.5, 1.0) if C.get_codec(n).uses_ratio else (0.0,))]


@lru_cache(maxsize=None)
def rows(elem, H, dtype, nonfinite=False):
    """([10, H], importance): tie / saturation rows (two walks), zero, denormal, massive (NaN / Inf), Gaussian rows."""
    g = torch.Generator().manual_seed(H)
    u = M.unit_rows(H)
    x = torch.cat([M.tie_rows(elem, H)[0], M.tie_rows(elem, H, 128)[0], u if nonfinite else u[[0, 2, 3]],
                   torch.randn(1, H, generator=g)])[:B * S]
    return x.to(dtype), torch.rand(B, S, generator=g)


def bits(t): return t.view(torch.int16 if t.dtype == BF16 else torch.int32)   # noqa: E704


@pytest.mark.parametrize("H", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("elem", list(M.ELEMS))
@pytest.mark.parametrize("name,ratio", CASES)
def test_gpu_equals_cpu(name, ratio, elem, dtype, H):
    spec = C.with_mx_elem(C.get_codec(name), elem)
    x, imp = rows(elem, H, dtype)
    m_cpu, L = C.encode(x, spec, B, S, ratio, imp)
    m_gpu, L2 = C.encode(x.to(DEV), spec, B, S, ratio, imp.to(DEV))
    assert L2 == L and M.ELEMS[elem][0] in (L.hi_fmt, L.lo_fmt)
    assert torch.equal(m_gpu.cpu(), m_cpu), f"{(m_gpu.cpu() != m_cpu).sum().item()} bytes differ"
    assert torch.equal(bits(C.decode(m_gpu, spec, L, dtype).cpu()), bits(C.decode(m_cpu, spec, L, dtype)))


@pytest.mark.parametrize("elem", list(M.ELEMS))
def test_nonfinite_blocks_and_foreign_messages(elem):
    """Only the code bytes of the NaN and the Inf block may differ from the CPU's; a foreign header decodes to NaN."""
    H, spec = 544, C.with_mx_elem(C.get_codec("mxfp4"), elem)
    x, _ = rows(elem, H, F32, True)
    m_cpu, L = C.encode(x, spec, B, S)
    m_dev, _ = C.encode(x.to(DEV), spec, B, S)
    m_gpu, end = m_dev.cpu(), L.off_hi + B * S * L.row_bytes(L.hi_fmt)
    (c_cpu, s_cpu), (c_gpu, s_gpu) = M.row_codes(m_cpu[L.off_hi:end], H), M.row_codes(m_gpu[L.off_hi:end], H)
    bad = (s_cpu == 255).repeat(32, axis=1)
    assert (s_cpu == 255).sum() == 2 and (s_cpu == s_gpu).all() and (c_cpu == c_gpu)[~bad].all()
    assert torch.equal(m_gpu[:L.off_hi], m_cpu[:L.off_hi]) and torch.equal(m_gpu[end:], m_cpu[end:])
    y, y_cpu = C.decode(m_dev, spec, L, F32).cpu(), C.decode(m_cpu, spec, L, F32)
    assert torch.equal(y.isnan(), torch.tensor(bad)) and torch.equal(bits(y)[~y.isnan()], bits(y_cpu)[~y.isnan()])
    m_dev[28:32] = 0
    m_dev[28] = W.FMT_MXFP4                                  # what the header of an unmodified mxfp4 message says
    assert bool(C.decode(m_dev, spec, L, F32).isnan().all())


def test_unsupported_combinations_are_rejected():
    """6-bit rows next to 16-bit wire or rotated group rows: hipErrorInvalidValue (1), and nothing is launched."""
    from llm_inference_in_distributed_edge_networks_amd.ops import _native
    H = 128
    L = C.layout(C.with_mx_elem(C.get_codec("mxfp4"), "e2m3"), B, S, H, 0, F32)
    x = torch.ones(B * S, H, device=DEV)
    for fmt6 in W.MX6_FORMATS:
        for other in (W.FMT_F16, W.FMT_F16S, W.FMT_GRPR):
            for hi, lo in ((fmt6, other), (other, fmt6)):
                for entry, x_f32 in (("edge_pack", 1), ("edge_pack", 0), ("edge_unpack", 1), ("edge_unpack", 0)):
                    msg = torch.full((1 << 14,), 0xAB, dtype=torch.uint8, device=DEV)
                    out = torch.full((B * S, H), 7.0, dtype=F32, device=DEV)
                    rc = getattr(_native.lib(), entry)(
                        (x if entry == "edge_pack" else out).data_ptr(), msg.data_ptr(), L.off_mask, L.off_scale, L.off_hi,
                        L.off_lo, -1, 0, B, S, H, 0, hi, lo, W.SC_NONE, 0, 0, 0, 1024, x_f32, _native.stream())
                    torch.cuda.synchronize()
                    assert rc == 1 and bool((msg == 0xAB).all()) and bool((out == 7.0).all()), (entry, hi, lo, rc)


def test_pipeline_in_a_captured_graph():
    """E2M3 lo rows at a LocalPipeline boundary: graph replays equal eager, counted bytes are the modified layout's."""
    from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
    from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
    from llm_inference_in_distributed_edge_networks_amd.models import TINY_QWEN2 as cfg, DecoderLM
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan
    model = DecoderLM.random_init(cfg, 1, std=0.05, device=torch.device(DEV), dtype=F32)
    ids = synthetic_stream(1000, cfg.vocab_size, 3)
    bl = [b.to(DEV) for b in batches(ids, sliding_windows(1000, 200, 32), 5) if b.B == 5][:4]
    plan, bcfg = PipelinePlan.from_split_layers(cfg.num_layers, [1]), BoundaryConfig("mixed_mxfp4_mxfp8", 0.5, mx_elem="e2m3")
    graph, eager = LocalPipeline(model, plan, bcfg), LocalPipeline(model, plan, bcfg, use_graphs=False)
    with torch.no_grad():
        for b in bl:                                         # eager, capture + replay, replay, replay
            assert torch.equal(graph.run_batch(b).clone(), eager.run_batch(b))
    assert len(bl) == 4 and graph.graphs.graphs, "nothing was captured"
    L = C.layout(bcfg.spec, 5, bl[0].S, cfg.hidden_size, W.num_lo(bcfg.spec, 0.5, bl[0].S), F32)
    assert L.lo_fmt == W.FMT_MXFP6 and graph.wire_bytes_per_token()[0] == L.total / (5 * bl[0].S)
