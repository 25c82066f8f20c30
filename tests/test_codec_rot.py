"""rgroup_rot: head-group rows quantized in the basis of the orthonormal 64-point Walsh-Hadamard transform (FMT_GRPR),
CPU oracle (codec/wire.py) and its way through the sweep engine, the pipeline runtime and the experiment drivers."""
import hashlib
import json

import pytest
import torch

from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

FP_PLAN = (2, 4, 8, 4, 4, 2, 8, 4, 4, 4, 2, 8, 4, 4)     # the plan of test_codec.WIRE_FINGERPRINTS


def rot(plan=None):
    spec = C.get_codec("rgroup_rot")
    return spec if plan is None else W.with_plan(spec, plan)


def massive(seed=0, n=256, H=896):
    """The prototype input: randn with channel 0 of every 64-channel group x 100; also the plain Gaussian."""
    torch.manual_seed(seed)
    x = torch.randn(n, H)
    xm = x.clone()
    xm[:, ::64] *= 100
    return x, xm


def mse(x, name, bits):
    spec = W.with_plan(C.get_codec(name), (bits,) * (x.shape[1] // 64))
    y, _ = C.fake_quant(x, spec, 1, x.shape[0])
    return float(((y - x) ** 2).mean())


def test_codec_is_registered():
    spec = C.get_codec("rgroup_rot")
    assert (spec.cid, spec.hi_fmt, spec.lo_fmt, spec.scale_mode) == (17, W.FMT_GRPR, W.FMT_GRPR, W.SC_NONE)
    assert W.FMT_GRPR == 8 and not spec.uses_ratio and not spec.needs_importance and W.needs_plan(spec)
    assert len({s.cid for s in W.CODECS.values()}) == len(W.CODECS)
    # no plan: 4 bits everywhere, as rgroup
    assert C.layout(spec, 2, 8, 256, 0, torch.float32).plan == (4, 4, 4, 4)
    with pytest.raises(ValueError):
        C.layout(spec, 2, 8, 96, 0, torch.float32)


@pytest.mark.parametrize("plan", [None, FP_PLAN, (2, 3, 4, 5, 6, 8, 2, 3, 4, 5, 6, 8, 4, 8)])
def test_message_bytes_equal_rgroup(plan):
    for dtype in (torch.float32, torch.bfloat16):
        a, b = rot(plan), C.get_codec("rgroup") if plan is None else W.with_plan(C.get_codec("rgroup"), plan)
        assert C.message_bytes(a, 3, 100, 896, 0.5, dtype) == C.message_bytes(b, 3, 100, 896, 0.5, dtype)
        La, Lb = C.layout(a, 3, 100, 896, 0, dtype), C.layout(b, 3, 100, 896, 0, dtype)
        assert La.row_bytes(W.FMT_GRPR) == Lb.row_bytes(W.FMT_GRP) and La.off_plan == Lb.off_plan


def test_wire_fingerprint():
    """The message of the WIRE_FINGERPRINTS input (test_codec.py), pinned to the CPU oracle's bytes."""
    torch.manual_seed(0)
    B, S, H = 2, 128, 896
    x = (torch.randn(B * S, H) * torch.logspace(-2, 2, H)).float()
    imp = torch.rand(B, S)
    msg, L = W.encode(x, rot(FP_PLAN), B, S, 0.5, imp)
    assert msg.numel() == 141392
    assert hashlib.sha1(msg.numpy().tobytes()).hexdigest()[:16] == "eefd9414a770af14"
    hdr = msg[:32].view(torch.int32).tolist()
    assert hdr[:3] == [W.MAGIC, W.VERSION, 17] and hdr[7] == W.FMT_GRPR
    assert bytes(msg[L.off_plan:L.off_plan + 14].tolist()) == bytes(FP_PLAN)
    # the header and plan aside, the rotation changes the rows: not rgroup's message
    ref, _ = W.encode(x, W.with_plan(C.get_codec("rgroup"), FP_PLAN), B, S, 0.5, imp)
    assert not torch.equal(msg[L.off_hi:], ref[L.off_hi:])


def test_transform_is_an_involution():
    g = torch.Generator().manual_seed(1)
    xi = torch.randint(-1000, 1000, (37, 192), generator=g).float()       # every partial sum < 2^24: exact
    assert torch.equal(W.hadamard64(W.hadamard64(xi)), xi)
    x = torch.randn(37, 192, generator=g)
    assert (W.hadamard64(W.hadamard64(x)) - x).abs().max() <= 1e-6
    # orthonormal: the group norms are kept; symmetric Sylvester matrix: row 1 is +-1 alternating
    y = W.hadamard64(x)
    assert torch.allclose(y.view(37, 3, 64).norm(dim=-1), x.view(37, 3, 64).norm(dim=-1), rtol=1e-5)
    e = torch.zeros(1, 64)
    e[0, 1] = 8.0
    assert W.hadamard64(e)[0].tolist() == [1.0, -1.0] * 32


def test_error_bound_every_width():
    """Per row and group ||x' - x||_2 <= 4 step: every code is within step / 2 of y, and the orthonormal inverse
    keeps the 2-norm of the 64 code errors, sqrt(64) step / 2."""
    plan = W.GROUP_BITS                                   # every width, non-uniform
    n, H = 96, 64 * len(plan)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, H, generator=g) * 2
    x[:, 64:128] *= 30
    x[:, 200] *= 100
    y, nb = C.fake_quant(x, rot(plan), 1, n)
    assert nb == C.message_bytes(rot(plan), 1, n, H, 0.0, torch.float32)
    yr = W.hadamard64(x).view(n, len(plan), 64)
    qmax = torch.tensor([(1 << (b - 1)) - 1 for b in plan], dtype=torch.float32)
    step = yr.abs().amax(-1) / qmax
    err = (y - x).view(n, len(plan), 64).norm(dim=-1)
    assert (err <= 4 * step * (1 + 1e-5) + 1e-6).all(), (err / step).max(0).values
    assert (err > 0).any(0).all()                          # and it does quantize every group


@pytest.mark.parametrize("bits", W.GROUP_BITS)
def test_single_channel_rows_are_exact(bits):
    """One non-zero channel per group: |y| is the same in every channel, every code is +-qmax, the integer inverse
    transform cancels exactly everywhere else and returns 64 qmax at the channel."""
    G = 5
    g = torch.Generator().manual_seed(3)
    x = torch.zeros(40, 64 * G)
    ch = torch.randint(0, 64, (40, G), generator=g) + 64 * torch.arange(G)
    val = torch.randn(40, G, generator=g) * 7
    x.scatter_(1, ch, val)
    y, _ = C.fake_quant(x, rot((bits,) * G), 1, 40)
    got = y.gather(1, ch)
    assert torch.equal(y.scatter(1, ch, 0.0), torch.zeros_like(y))
    ulp = torch.ldexp(torch.ones(()), torch.frexp(val.abs())[1] - 24)
    assert ((got - val).abs() <= 4 * ulp).all(), ((got - val).abs() / ulp).max()


def test_outlier_behaviour():
    """MSE(rgroup) / MSE(rgroup_rot), uniform plans: a massive channel per group gains at 4 and 8 bits; nothing is
    lost on a plain Gaussian.  (At 3 bits the rotation loses on the massive-channel input - 0.41 - because rgroup
    then zeroes the small channels and its error stays bounded by their variance.)"""
    x, xm = massive()
    assert mse(xm, "rgroup", 8) / mse(xm, "rgroup_rot", 8) >= 10          # prototype: 47.9
    assert mse(xm, "rgroup", 4) / mse(xm, "rgroup_rot", 4) >= 1.5         # prototype: 2.17
    for bits in (4, 8):
        assert 0.95 <= mse(x, "rgroup", bits) / mse(x, "rgroup_rot", bits) <= 1.05    # prototype: 1.014


@pytest.mark.parametrize("bad", [0, 7, 255])
@pytest.mark.parametrize("name", ["rgroup", "rgroup_rot"])
def test_corrupt_plan_decodes_to_nan_from_that_group(name, bad):
    """The CPU decoder reads the widths from the message's plan bytes as the GPU does, for plain and rotated head-group
    rows: a width outside GROUP_BITS gives NaN from that group on and leaves the groups before it intact."""
    B, S, H = 2, 16, 512
    x = torch.randn(B * S, H, generator=torch.Generator().manual_seed(4))
    spec = W.with_plan(C.get_codec(name), (4,) * 8)
    msg, L = C.encode(x, spec, B, S)
    good = C.decode(msg, spec, L, torch.float32)
    assert torch.isfinite(good).all()
    msg = msg.clone()
    msg[L.off_plan + 3] = bad
    y = C.decode(msg, spec, L, torch.float32)
    assert torch.equal(y[:, :192], good[:, :192]) and torch.isnan(y[:, 192:]).all()
    # a valid but wider width whose streams run past the row's code bytes: NaN from the group that overruns
    msg[L.off_plan + 3] = 8
    y = C.decode(msg, spec, L, torch.float32)
    assert torch.isfinite(y[:, :448]).all() and torch.isnan(y[:, 448:]).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fake_quant(dtype):
    B, S, H = 2, 24, 256
    x = (torch.randn(B * S, H, generator=torch.Generator().manual_seed(5)) * 2).to(dtype)
    y, nb = C.fake_quant(x, rot((8, 4, 5, 4)), B, S, 0.5, torch.rand(B, S))
    assert y.dtype == dtype and y.shape == x.shape and torch.isfinite(y).all()
    assert nb == C.message_bytes(rot((8, 4, 5, 4)), B, S, H, 0.5, dtype)
    # rounding error of rms step / sqrt(12) per channel, step = max|y| / 7 at 4 bits, max of 64 Gaussians < 4.5 sigma:
    # below 4.5 / (7 sqrt(12)) = 0.19 of the rms even if every group were 4 bits wide
    rel = (y.float() - x.float()).norm() / x.float().norm()
    assert 0 < rel < 0.19


@pytest.mark.parametrize("skewed", [False, True])
def test_sweep_equals_split_runner(skewed):
    """Sweep engine == pipeline runtime on tiny-qwen2, uniform plans and plans allocated from a skewed channel-group
    relevance table (the unrotated table: what both are fed)."""
    from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
    from llm_inference_in_distributed_edge_networks_amd.eval.sweep import SweepConfig, SweepEngine, run_sweep
    from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
    from llm_inference_in_distributed_edge_networks_amd.models import TINY_QWEN2, DecoderLM
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan
    m = DecoderLM.random_init(TINY_QWEN2, 0, std=0.06)
    tok, wins = synthetic_stream(700, 512, 1), sliding_windows(700, 128, 32)
    G = TINY_QWEN2.hidden_size // 64
    grel = None
    if skewed:
        grel = torch.rand(TINY_QWEN2.num_layers, G, generator=torch.Generator().manual_seed(3))
        grel[1] = torch.tensor([1.0] + [0.02] * (G - 1))
    sc = SweepConfig(["regular_importance"], [0, 2], [1], codec="rgroup_rot", group_relevance=grel, group_avg_bits=4.0)
    eng = SweepEngine(m, sc)
    res = run_sweep(eng, batches(tok, wins, 4))
    for li, L in enumerate([0, 2]):
        bc = BoundaryConfig("rgroup_rot", 1, "regular_importance", group_relevance=grel, group_avg_bits=4.0)
        pipe = LocalPipeline(m, PipelinePlan.from_split_layers(4, [L]), bc)
        assert pipe.stages[0].spec_out.plan == eng._spec_at("rgroup_rot", L).plan
        assert pipe.stages[0].spec_out.lo_fmt == W.FMT_GRPR
        ppl = pipe.evaluate(batches(tok, wins, 4)).ppl()
        assert abs(ppl - res["avg_ppl_results"][0][li][0]) / ppl < 1e-6, L
        assert abs(pipe.wire_bytes_per_token()[0] - res["wire_bytes_per_token"][0][li][0]) < 1e-6
    assert eng._spec_at("rgroup_rot", 0).plan == ((8, 4, 2, 2) if skewed else (4,) * G)


def test_pipeline_driver_wire_bytes_equal_rgroup(tmp_path):
    from test_experiments_cpu import run_main
    res = {}
    for codec in ("rgroup", "rgroup_rot"):
        (tmp_path / codec).mkdir()
        d = run_main("Pipeline", {"model": "tiny-qwen2", "num_stages": 2, "codec": codec, "methods": ["last_row"],
                                  "ratios": [0, 1], "max_length": 64}, tmp_path / codec)
        res[codec] = json.loads((d / "pipeline_results.json").read_text())["results"]["last_row"]
    for r in ("0", "1"):
        assert res["rgroup_rot"][r]["wire_bytes_per_token"] == res["rgroup"][r]["wire_bytes_per_token"]
        assert res["rgroup_rot"][r]["ppl"] > 0
    assert res["rgroup_rot"]["1"]["ppl"] != res["rgroup"]["1"]["ppl"]
