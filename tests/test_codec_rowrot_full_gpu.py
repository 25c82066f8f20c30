"""Row-rotated per-token int rows on the RF kernels (csrc/codec.hip rot_full_row): the GPU's message and decode are the
CPU oracle's bit for bit - on non-integer rows too, which is the check of the lane / chunk maps, of the LDS column
stage and of the 28-term accumulation order."""
import pytest
import torch

from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W
from test_codec_outliers import CASES
from test_codec_outliers_gpu import BF16, DEV, F32, bits
from test_codec_rowrot import B, IMP, RATIO, S, hard_rows

pytestmark = pytest.mark.gpu
full = lambda n: C.with_row_rot(C.get_codec(n), "full")   # noqa: E731


# 256: lane ^ 16, half the wave idle; 512: lane ^ 32; 1024: one chunk stage; 4096: NCH 8, three chunk stages; 896: two
# lanes per column, chunk 1 partly live; 1792: one lane per column; 3584: two columns per lane, 7 of 8 chunks live
@pytest.mark.parametrize("H", [256, 512, 1024, 4096, 896, 1792, 3584])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,sel", CASES)
def test_gpu_equals_cpu(name, sel, dtype, H):
    spec = full(name)
    x = hard_rows(H)
    x[6:] = torch.randn(4, H, generator=torch.Generator().manual_seed(H)) * (1 + 40 * (torch.arange(H) % 97 == 5))
    x = x.to(dtype)
    finite = x.clone()
    finite[3:6] = x[[0, 1, 9]].flip(1)                       # without the NaN / Inf / overflow rows: every byte
    m_cpu, L = C.encode(finite, spec, B, S, RATIO, IMP, selection=sel)
    m_gpu, L2 = C.encode(finite.to(DEV), spec, B, S, RATIO, IMP.to(DEV), selection=sel)
    assert L2 == L and torch.equal(m_gpu.cpu(), m_cpu), f"{(m_gpu.cpu() != m_cpu).sum().item()} bytes differ"
    assert torch.equal(bits(C.decode(m_gpu, spec, L, dtype).cpu()), bits(C.decode(m_cpu, spec, L, dtype)))
    y_cpu = C.decode(C.encode(x, spec, B, S, RATIO, IMP, selection=sel)[0], spec, L, dtype)
    y = C.decode(C.encode(x.to(DEV), spec, B, S, RATIO, IMP.to(DEV), selection=sel)[0], spec, L, dtype).cpu()
    ok = y_cpu.isfinite()                                    # with them: non-finite on both sides, the rest bit for bit
    assert torch.equal(y.isfinite(), ok) and torch.equal(bits(y)[ok], bits(y_cpu)[ok])


def test_unsupported_combinations_are_rejected():   # hipErrorInvalidValue (1), and nothing is launched
    from llm_inference_in_distributed_edge_networks_amd.ops import _native
    L = C.layout(full("int4_token"), B, S, 256, 2, F32)
    for H, hi, mode in ((384, W.FMT_F32, W.SC_TOKEN), (256, W.FMT_F32, W.SC_WINDOW), (256, W.FMT_INT8R, W.SC_TOKEN),
                        (256, W.FMT_INT4O, W.SC_TOKEN)):
        for entry, x_f32 in (("edge_pack", 1), ("edge_pack", 0), ("edge_unpack", 1), ("edge_unpack", 0)):
            msg = torch.full((1 << 14,), 0xAB, dtype=torch.uint8, device=DEV)
            x = torch.full((B * S, 384), 7.0, dtype=F32, device=DEV)
            rc = getattr(_native.lib(), entry)(x.data_ptr(), msg.data_ptr(), L.off_mask, L.off_scale, L.off_hi, L.off_lo,
                                               -1, -1, B, S, H, 2, hi, W.FMT_INT4F, mode, 0, 7, 0, 0, x_f32,
                                               _native.stream())
            torch.cuda.synchronize()
            assert rc == 1 and bool((msg == 0xAB).all()) and bool((x == 7.0).all()), (entry, H, hi, mode, rc)


def test_pipeline_boundary_equals_cpu_decode():   # stage 1's input on the GPU: the CPU decode of the same message
    from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
    from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
    from llm_inference_in_distributed_edge_networks_amd.models import TINY_QWEN2 as cfg, DecoderLM
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan
    plan, bcfg = PipelinePlan.from_split_layers(cfg.num_layers, [1]), BoundaryConfig("mixed_int4_int8", 0.5, row_rot="full")
    gpu, cpu = (LocalPipeline(DecoderLM.random_init(cfg, 1, std=0.05, device=torch.device(d), dtype=F32), plan, bcfg)
                for d in (DEV, "cpu"))
    b = next(batches(synthetic_stream(1000, cfg.vocab_size, 3), sliding_windows(1000, 200, 32), 3))
    with torch.no_grad():
        x0, imp, _ = gpu.stages[0].run(b.to(DEV))
        msg, L = gpu.stages[0].encode(x0, b.to(DEV), imp)
        got = C.decode(msg, gpu.stages[1].spec_in, gpu.stages[1].layout_in(b.to(DEV)), F32)
        want = C.decode(msg.cpu(), cpu.stages[1].spec_in, cpu.stages[1].layout_in(b), F32)
        assert torch.isfinite(gpu.run_batch(b.to(DEV))).all()
    assert L.hi_fmt == W.FMT_INT8F and L.lo_fmt == W.FMT_INT4F and 0 < L.k < L.S
    assert torch.equal(bits(got.cpu()), bits(want)) and want.isfinite().all()
