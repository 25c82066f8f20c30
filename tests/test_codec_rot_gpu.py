"""rgroup_rot (FMT_GRPR rows: head groups quantized in the 64-point Walsh-Hadamard basis) on the GPU: the ROT
instantiations of pack_kernel / unpack_kernel against the CPU oracle of codec/wire.py, byte for byte and bit for bit."""
from functools import lru_cache

import pytest
import torch

from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import plan as P
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (1, 5, 64): one group, 56 idle lanes, a partial 4-row block; (2, 33, 576): the second chunk holds a single group;
# (1, 16, 4096): 8 chunks per lane
SHAPES = [(1, 5, 64), (2, 33, 576), (3, 200, 896), (1, 16, 4096)]
PLANS = ["uniform4", "all_widths", "mse"]


def plan_of(kind, H):
    G = H // 64
    if kind == "uniform4":
        return (4,) * G
    if kind == "all_widths":
        return tuple(W.GROUP_BITS[g % len(W.GROUP_BITS)] for g in range(G))
    # a few dominant groups: the MSE allocation is non-uniform (one group: 4 bits)
    return P.allocate_group_bits([100.0 if g % 5 == 0 else 1.0 for g in range(G)], 4.0, model="mse")


def spec_of(kind, H):
    return W.with_plan(C.get_codec("rgroup_rot"), plan_of(kind, H))


def activations(B, S, H, dtype=torch.float32):
    """randn * 2 with one loud group (x 30) and one massive channel (x 100)."""
    x = torch.randn(B * S, H, generator=torch.Generator().manual_seed(B * 1000 + S)) * 2
    g = (H // 64) // 2
    x[:, 64 * g:64 * g + 64] *= 30
    x[:, H - 7] *= 100
    return x.to(dtype)


@lru_cache(maxsize=None)
def cpu_reference(B, S, H, kind, dtype):
    """CPU message and fp32 decode of the (dtype-rounded) input; shared by the tests, never modified."""
    x = activations(B, S, H, dtype)
    spec = spec_of(kind, H)
    msg, L = C.encode(x.float(), spec, B, S)
    return x, msg, L, C.decode(msg, spec, L, torch.float32)


@pytest.mark.parametrize("B,S,H", SHAPES)
@pytest.mark.parametrize("kind", PLANS)
def test_gpu_equals_cpu_fp32(B, S, H, kind):
    spec = spec_of(kind, H)
    assert kind != "mse" or H == 64 or len(set(spec.plan)) > 1
    x, m_cpu, L, y_cpu = cpu_reference(B, S, H, kind, torch.float32)
    m_gpu, L2 = C.encode(x.to(DEV), spec, B, S)
    assert L2 == L
    assert torch.equal(m_gpu.cpu(), m_cpu), f"{(m_gpu.cpu() != m_cpu).sum().item()} bytes differ"
    assert torch.equal(C.decode(m_gpu, spec, L, torch.float32).cpu(), y_cpu)
    # cross-decode: GPU decode of the CPU's bytes, CPU decode of the GPU's bytes
    assert torch.equal(C.decode(m_cpu.to(DEV), spec, L, torch.float32).cpu(), y_cpu)
    assert torch.equal(C.decode(m_gpu.cpu(), spec, L, torch.float32), y_cpu)
    assert torch.isfinite(y_cpu).all()


@pytest.mark.parametrize("B,S,H", [(2, 33, 576), (3, 200, 896)])
@pytest.mark.parametrize("kind", ["all_widths", "mse"])
def test_gpu_equals_cpu_bf16(B, S, H, kind):
    """bf16 activations: the bytes of the CPU oracle run on the bf16-rounded input; the decode into bf16 is the CPU's
    fp32 decode rounded to bf16."""
    spec = spec_of(kind, H)
    x, m_cpu, L, y_cpu = cpu_reference(B, S, H, kind, torch.bfloat16)
    m_gpu, _ = C.encode(x.to(DEV), spec, B, S)
    assert torch.equal(m_gpu.cpu(), m_cpu)
    assert torch.equal(C.decode(m_gpu, spec, L, torch.bfloat16).cpu(), y_cpu.to(torch.bfloat16))
    assert torch.equal(C.decode(m_gpu, spec, L, torch.float32).cpu(), y_cpu)


@pytest.mark.parametrize("bad", [0, 7, 255])
def test_gpu_rejects_corrupt_plan(bad):
    """A plan byte outside GROUP_BITS: NaN from that group on (also in the second chunk), the groups before it
    intact - the same as the CPU decoder gives for those bytes."""
    B, S, H = 2, 33, 576
    spec = spec_of("uniform4", H)
    x, m_cpu, L, y_cpu = cpu_reference(B, S, H, "uniform4", torch.float32)
    msg = m_cpu.clone()
    msg[L.off_plan + 3] = bad
    y = C.decode(msg.to(DEV), spec, L, torch.float32).cpu()
    torch.cuda.synchronize()
    assert torch.equal(y[:, :192], y_cpu[:, :192])
    assert torch.isnan(y[:, 192:]).all()
    y_bad = C.decode(msg, spec, L, torch.float32)          # the CPU decode of the same corrupted bytes
    assert torch.equal(torch.isnan(y), torch.isnan(y_bad))
    assert torch.equal(y[~torch.isnan(y)], y_bad[~torch.isnan(y_bad)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_output_element_is_written(dtype):
    B, S, H = 2, 33, 576
    spec = spec_of("all_widths", H)
    _, m_cpu, L, _ = cpu_reference(B, S, H, "all_widths", torch.float32)
    msg = m_cpu.to(DEV)
    zero = torch.zeros(B * S, H, dtype=dtype, device=DEV)
    ones = torch.empty(B * S, H, dtype=dtype, device=DEV)
    ones.view(torch.uint8).fill_(0xFF)
    C.decode(msg, spec, L, out=zero)
    C.decode(msg, spec, L, out=ones)
    assert torch.equal(zero.view(torch.uint8), ones.view(torch.uint8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graph_replay_equals_eager(dtype):
    from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
    from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
    from llm_inference_in_distributed_edge_networks_amd.models import TINY_QWEN2, DecoderLM
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan
    tok, wins = synthetic_stream(1500, 512, 4), sliding_windows(1500, 256, 32)
    m = DecoderLM.random_init(TINY_QWEN2, 1, device="cuda", dtype=dtype, std=0.05)
    plan = PipelinePlan.from_split_layers(TINY_QWEN2.num_layers, [1, 2])
    bc = BoundaryConfig("rgroup_rot", 1.0, "last_row")
    eager = LocalPipeline(m, plan, bc, use_graphs=False)
    graphed = LocalPipeline(m, plan, bc, use_graphs=True)
    assert eager.stages[0].spec_out.lo_fmt == W.FMT_GRPR
    bl = [b.to("cuda") for b in batches(tok, wins, 4)]
    for _ in range(3):          # eager warmup, capture, replay
        for b in bl:
            e = eager.run_batch(b).clone()
            g = graphed.run_batch(b).clone()
            assert torch.isfinite(g).all() and torch.equal(e, g)
    assert graphed.graphs.graphs, "nothing was captured"
    assert eager.wire_bytes_per_token() == graphed.wire_bytes_per_token()


def test_pack_unpack_deterministic():
    B, S, H = 64, 512, 896
    spec = spec_of("all_widths", H)
    x = (torch.randn(B * S, H, generator=torch.Generator(DEV).manual_seed(7), device=DEV) * 2)
    x[:, 70] *= 100
    m1, L = C.encode(x, spec, B, S)
    m2, _ = C.encode(x, spec, B, S)
    assert torch.equal(m1, m2)
    y1 = C.decode(m1, spec, L, torch.float32)
    y2 = C.decode(m2, spec, L, torch.float32)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)) and torch.isfinite(y1).all()
