"""Variable-k (top-rho) boundary messages on the GPU (csrc/codec.hip: select_sort_kernel's block scan, kvar_prefix,
the moving hi section of pack_kernel / unpack_kernel) against the CPU codec (codec.wire._encode_cpu / _decode_cpu),
byte for byte, and the pipeline / sweep runtimes on top of them (in-graph payload accounting, graph replay)."""
import pytest
import torch

import helpers as T
from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W
from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
from llm_inference_in_distributed_edge_networks_amd.eval.sweep import SweepConfig, SweepEngine, SweepMethod, run_sweep
from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
from llm_inference_in_distributed_edge_networks_amd.models import TINY_NEOX, TINY_QWEN2, DecoderLM
from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
_IDS = {"ids": lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")}


def _diff(a, b):
    ne = (a != b).nonzero()
    return f"{ne.numel()} of {a.numel()} bytes differ, first at {int(ne[0]) if ne.numel() else -1}"


def _bits(y):
    """The tensor's bytes (bit equality also tells -0 from +0 and compares NaN payloads)."""
    return y.cpu().contiguous().view(torch.uint8)


def check_message(x, spec, B, S, ks_ref, m_cpu, L, m_gpu, L_gpu):
    """GPU message == CPU message on the payload bytes, and the four encode x decode pairings give the same bits.
    ``x`` on the CPU in the dtype under test; ``m_cpu`` the oracle's message of the same (rounded) values."""
    assert L_gpu == L
    mg = m_gpu.cpu()
    assert W.message_k(mg, L).tolist() == [int(k) for k in ks_ref]
    payload = W.message_payload(m_cpu, L)
    assert W.message_payload(mg, L) == payload <= L.total
    assert torch.equal(mg[:payload], m_cpu[:payload]), _diff(mg[:payload], m_cpu[:payload])
    y_cc = C.decode(m_cpu, spec, L, x.dtype)
    assert torch.isfinite(y_cc).all()
    y_gg = C.decode(m_gpu, spec, L, x.dtype)                   # GPU decode of the GPU message
    y_cg = C.decode(m_cpu.to(DEV), spec, L, x.dtype)           # GPU decode of the CPU message: unpack on its own
    y_gc = C.decode(mg, spec, L, x.dtype)                      # CPU decode of the GPU message: pack on its own
    for name, y in (("gpu(gpu)", y_gg), ("gpu(cpu)", y_cg), ("cpu(gpu)", y_gc)):
        assert torch.equal(_bits(y), _bits(y_cc)), f"decode {name}: {_diff(_bits(y), _bits(y_cc))}"


# ---- 2. message bytes and decode on inputs whose k is exact on both sides ----------------------------------------
@pytest.mark.parametrize("shape", T.KVAR_SHAPES, **_IDS)
@pytest.mark.parametrize("ratio", T.KVAR_RATIOS)
@pytest.mark.parametrize("dtype", DTYPES, **_IDS)
@pytest.mark.parametrize("codec", T.KVAR_CODECS)
def test_top_rho_message_equals_cpu(codec, dtype, ratio, shape):
    B, S, H = shape
    spec = T.kvar_spec(codec, H)
    imp = T.dyadic_importance(B, S, T.kvar_seed(B, S))
    x = T.kvar_activations(B, S, H, T.kvar_seed(B, S) + 1, dtype)
    m_cpu, L = C.encode(x, spec, B, S, ratio, imp, selection="top_rho")
    m_gpu, L_gpu = C.encode(x.to(DEV), spec, B, S, ratio, imp.to(DEV), selection="top_rho")
    assert L.kvar
    check_message(x, spec, B, S, W.top_rho_k(imp, 1.0 - ratio), m_cpu, L, m_gpu, L_gpu)


@pytest.mark.parametrize("shape", [(70, 37, 128), (5, 200, 896)], **_IDS)
@pytest.mark.parametrize("ratio", T.KVAR_RATIOS)
@pytest.mark.parametrize("dtype", DTYPES, **_IDS)
@pytest.mark.parametrize("codec", T.KVAR_CODECS)
def test_fixed_k_message_equals_cpu_many_windows(codec, dtype, ratio, shape):
    """The fixed-k layout at the same shapes: B > 64 and H = 128 (one 64-lane chunk, a quarter used)."""
    B, S, H = shape
    spec = T.kvar_spec(codec, H)
    imp = T.dyadic_importance(B, S, T.kvar_seed(B, S))
    x = T.kvar_activations(B, S, H, T.kvar_seed(B, S) + 1, dtype)
    m_cpu, L = C.encode(x, spec, B, S, ratio, imp)
    m_gpu, L_gpu = C.encode(x.to(DEV), spec, B, S, ratio, imp.to(DEV))
    assert not L.kvar and 0 < L.k == int(ratio * S) < S
    check_message(x, spec, B, S, [L.k] * B, m_cpu, L, m_gpu, L_gpu)


# ---- 3. realistic importance: the oracle message is built from the k the GPU chose -------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_IDS)
@pytest.mark.parametrize("codec", ["mixed_int4_int8", "ref_int4_global", "mxfp4_keep"])
def test_top_rho_softmax_importance(codec, dtype):
    B, S, H, ratio = 6, 200, 896, 0.4
    spec = T.kvar_spec(codec, H)
    imp = torch.softmax(torch.randn(B, S, generator=torch.Generator().manual_seed(S * 10 + 40)) * 3, -1)
    x = T.kvar_activations(B, S, H, 7, dtype)
    m_gpu, L = C.encode(x.to(DEV), spec, B, S, ratio, imp.to(DEV), selection="top_rho")
    ks = W.message_k(m_gpu.cpu(), L)
    ref_k = W.top_rho_k(imp, 1.0 - ratio)
    desc = torch.sort(imp, dim=1, stable=True).values.flip(1).double()
    excl = torch.cumsum(desc, 1) - desc
    for b in range(B):
        if int(ks[b]) != int(ref_k[b]):
            # the rule of test_select_gpu.test_top_rho_equals_cpu: parallel fp32 scan vs fp64 sequential sums, the
            # cut may only move inside the run of positions whose exclusive mass is within 1e-5 of the threshold
            lo_keep, hi_keep = sorted((S - int(ks[b]), S - int(ref_k[b])))
            gap = (excl[b, lo_keep:hi_keep + 1] - (1.0 - ratio)).abs().max()
            assert gap < 1e-5, (b, int(ks[b]), int(ref_k[b]), float(gap))
    assert bool(((ks > 0) & (ks < S)).all())
    m_cpu = W._encode_cpu(x, spec, L, W.select_mask(imp, ks))
    check_message(x, spec, B, S, ks, m_cpu, L, m_gpu, L)


# ---- 4. a reused message buffer (what a graph replay does) -------------------------------------------------------
def _written_sections(spec, L, kt):
    """Byte ranges of a variable-k message that an encode writes.  Not in the list: the padding that rounds every
    section up to 16 bytes - in particular the up to 15 bytes between the last lo row and the hi section, which move
    with sum k and which the kernels never write (a fresh buffer has zeros there, a reused one whatever a row of
    the previous message left)."""
    B, S, H = L.B, L.S, L.H
    n_scale = {W.SC_TOKEN: B * S, W.SC_WINDOW: B, W.SC_CHANNEL: B * H, W.SC_NONE: 0}[spec.scale_mode]
    rl, rh = L.row_bytes(L.lo_fmt), L.row_bytes(L.hi_fmt)
    sec = {"header": (0, 32), "mask": (L.off_mask, L.off_mask + 4 * B * L.mw), "k": (L.off_kvec, L.off_kvec + 4 * B),
           "scales": (L.off_scale, L.off_scale + 4 * n_scale), "lo rows": (L.off_lo, L.off_lo + kt * rl),
           "hi rows": (L.hi_offset(kt), L.hi_offset(kt) + (B * S - kt) * rh)}
    if L.plan is not None:
        sec["plan"] = (L.off_plan, L.off_plan + len(L.plan))
    return sec


@pytest.mark.parametrize("dtype", DTYPES, **_IDS)
@pytest.mark.parametrize("codec", T.KVAR_CODECS)
def test_top_rho_reused_buffer(codec, dtype):
    B, S, H = 5, 200, 896
    spec = T.kvar_spec(codec, H)
    # first message: many lo rows (keep mass 0.25); second: few (keep mass 0.75, other importance and activations)
    imp1, imp2 = T.dyadic_importance(B, S, 11), T.dyadic_importance(B, S, 12)
    x1, x2 = T.kvar_activations(B, S, H, 13, dtype), T.kvar_activations(B, S, H, 14, dtype)
    L = C.layout(spec, B, S, H, -1, dtype, kvar=True)
    out = torch.full((L.total,), 0xFF, dtype=torch.uint8, device=DEV)
    m1, _ = C.encode(x1.to(DEV), spec, B, S, 0.75, imp1.to(DEV), out=out, selection="top_rho")
    kt1 = int(W.message_k(m1.cpu(), L).sum())
    m2, L2 = C.encode(x2.to(DEV), spec, B, S, 0.25, imp2.to(DEV), out=out, selection="top_rho")
    assert m2.data_ptr() == out.data_ptr() and L2 == L
    fresh, _ = C.encode(x2.to(DEV), spec, B, S, 0.25, imp2.to(DEV), selection="top_rho")
    kt2 = int(W.message_k(fresh.cpu(), L).sum())
    assert kt2 == int(W.top_rho_k(imp2, 0.75).sum()) and kt1 == int(W.top_rho_k(imp1, 0.25).sum())
    assert kt1 > kt2 + B * S // 4 and kt2 > 0         # the hi section moved down over former lo rows
    a, f = m2.cpu(), fresh.cpu()
    for name, (lo, hi) in _written_sections(spec, L, kt2).items():
        assert torch.equal(a[lo:hi], f[lo:hi]), f"{name}: {_diff(a[lo:hi], f[lo:hi])}"
    y, y_fresh = C.decode(m2, spec, L, dtype), C.decode(fresh, spec, L, dtype)
    assert torch.isfinite(y).all() and torch.equal(_bits(y), _bits(y_fresh))
    assert torch.equal(_bits(y), _bits(C.decode(a, spec, L, dtype)))        # and the CPU decoder on the reused bytes


# ---- 5. pipeline and sweep ---------------------------------------------------------------------------------------
TOK = synthetic_stream(1500, 512, 4)
WINS = sliding_windows(1500, 256, 32)


def _batches():
    return [b.to(DEV) for b in batches(TOK, WINS, 4)]


def _replay_equals_eager(cfg, dtype, bcfg):
    m = DecoderLM.random_init(cfg, 1, device=DEV, dtype=dtype, std=0.05)
    plan = PipelinePlan.from_split_layers(cfg.num_layers, [1, 2])
    eager = LocalPipeline(m, plan, bcfg, use_graphs=False)
    graphed = LocalPipeline(m, plan, bcfg, use_graphs=True)
    bl = _batches()
    for _ in range(3):          # eager first sighting, pre-capture run + capture + replay, replay
        for b in bl:
            e = eager.run_batch(b).clone()
            g = graphed.run_batch(b).clone()
            assert torch.isfinite(g).all() and torch.equal(e, g)
    assert graphed.graphs.graphs, "nothing was captured"
    # payload bytes are summed on the device inside the captured graph: every micro-batch counted exactly once
    assert eager.wire_bytes_per_token() == graphed.wire_bytes_per_token()
    return eager


@pytest.mark.parametrize("method", ["regular_importance", "last_row"])
@pytest.mark.parametrize("codec", ["mixed_int4_int8", "ref_int4_global"])
@pytest.mark.parametrize("ratio", [0.25, 0.75])
@pytest.mark.parametrize("dtype", DTYPES, **_IDS)
@pytest.mark.parametrize("cfg", [TINY_QWEN2, TINY_NEOX], ids=lambda c: c.name)
def test_top_rho_graph_replay_equals_eager(cfg, dtype, ratio, codec, method):
    eager = _replay_equals_eager(cfg, dtype, BoundaryConfig(codec, ratio, method, selection="top_rho"))
    for st in eager.stages[:-1]:
        assert st.bcfg.kvar and st.stats.kvar_bytes is not None and st.stats.wire_bytes == 0


@pytest.mark.parametrize("codec", ["mixed_int4_int8", "ref_int4_global"])
@pytest.mark.parametrize("dtype", DTYPES, **_IDS)
def test_top_rho_graph_replay_ratio_one(dtype, codec):
    """Keep mass 0: no importance is tracked and every window has k = S (the all-lo message, hi section empty)."""
    bcfg = BoundaryConfig(codec, 1.0, "regular_importance", selection="top_rho")
    assert bcfg.kvar and not bcfg.needs_importance(256)
    eager = _replay_equals_eager(TINY_QWEN2, dtype, bcfg)
    bl = _batches()
    for st in eager.stages[:-1]:
        want = sum(st.layout(b).payload_bytes(b.B * b.S) for b in bl)
        assert st.stats.totals() == (3.0 * want, 3.0 * sum(b.B * b.S for b in bl))


def test_top_rho_wire_bytes_equal_host_sum():
    """The device-side payload sum of a stage == message_payload of each of its messages, summed on the host."""
    m = DecoderLM.random_init(TINY_QWEN2, 1, device=DEV, dtype=torch.bfloat16, std=0.05)
    plan = PipelinePlan.from_split_layers(TINY_QWEN2.num_layers, [1, 2])
    bcfg = BoundaryConfig("mixed_int4_int8", 0.75, "regular_importance", selection="top_rho")
    st = LocalPipeline(m, plan, bcfg, use_graphs=False).stages[0]
    host, tokens, kt = 0, 0, 0
    for b in _batches():
        st.account(b)
        x, imp, _ = st.run(b)
        msg, L = st.encode(x, b, imp)
        assert L.kvar
        host += W.message_payload(msg.cpu(), L)
        tokens += b.B * b.S
        kt += int(W.message_k(msg.cpu(), L).sum())
    assert 0 < kt < tokens                                   # the messages are neither all hi nor all lo
    assert st.stats.totals() == (float(host), float(tokens))


def test_gpu_sweep_top_rho_equals_split_runner():
    """Top-rho rows of the sweep engine == the pipeline runtime with selection='top_rho', both on the GPU."""
    m = DecoderLM.random_init(TINY_QWEN2, 0, device=DEV, dtype=torch.bfloat16, std=0.05)
    rows = [SweepMethod("rho", "regular_importance", selection="top_rho"),
            SweepMethod("rho_last", "last_row", selection="top_rho")]
    ratios = [0.25, 0.75, 1.0]
    sc = SweepConfig(rows, [1], ratios, codec="mixed_int4_int8")
    res = run_sweep(SweepEngine(m, sc), batches(TOK, WINS, 4))
    for mi, meth in enumerate(["regular_importance", "last_row"]):
        for ri, r in enumerate(ratios):
            pipe = LocalPipeline(m, PipelinePlan.from_split_layers(4, [1]),
                                 BoundaryConfig("mixed_int4_int8", r, meth, selection="top_rho"), use_graphs=False)
            ppl = pipe.evaluate(batches(TOK, WINS, 4)).ppl()
            wire = pipe.wire_bytes_per_token()[0]
            assert abs(ppl - res["avg_ppl_results"][mi][0][ri]) / ppl < 1e-5, (meth, r)
            assert abs(wire - res["wire_bytes_per_token"][mi][0][ri]) / wire < 1e-5, (meth, r)
