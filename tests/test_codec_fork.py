"""codec.fake_quant_fork / fork_supported on CPU tensors: the stacked per-variant fake_quant (the oracle of
tests/test_codec_fork_gpu.py), the codecs it serves, its errors and its byte counts."""
import pytest
import torch

from llm_inference_in_distributed_edge_networks_amd import codec as C

FORKED = ("ref_int4_global", "int4_token", "int8_token", "int8_token_keep", "mixed_int4_int8", "mixed_int2_int8")
B, S, H = 2, 37, 96


def _inputs(dtype):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B * S, H, generator=g) * 2).to(dtype)
    imps = [torch.randn(B, S, generator=g), torch.rand(B, S, generator=g)]
    return x, imps, [(0, 0), (0, 5), (1, 5), (1, S - 1), (None, S), (None, 0)]


def test_fork_supported():
    assert {n for n, s in C.CODECS.items() if C.fork_supported(s, "ratio")} == set(FORKED)
    for n in FORKED:
        assert not C.fork_supported(C.get_codec(n), "top_rho")
    for n in ("ref_int4_global", "int4_token", "int8_token_keep"):
        for wire in ("bf16", "fp16", "fp16s"):
            assert not C.fork_supported(C.with_native_wire(C.get_codec(n), wire), "ratio")
    for n in ("mxfp4", "rgroup", "channel_8"):
        assert not C.fork_supported(C.get_codec(n), "ratio")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", FORKED)
def test_cpu_fork_is_the_per_variant_loop(name, dtype):
    spec = C.get_codec(name)
    x, imps, variants = _inputs(dtype)
    y, nbytes = C.fake_quant_fork(x, spec, B, S, variants, imps)
    assert y.shape == (len(variants) * B * S, H) and y.dtype == dtype
    for v, (src, k) in enumerate(variants):
        ref, nb = C.fake_quant(x, spec, B, S, importance=None if src is None else imps[src], k=k)
        assert torch.equal(y[v * B * S:(v + 1) * B * S], ref)
        ratio = {0: 0.0, 5: 5.5 / S, S - 1: (S - 0.5) / S, S: 1.0}[k]
        assert nbytes[v] == nb == C.message_bytes(spec, B, S, H, ratio, dtype)
    out = torch.empty_like(y)
    assert C.fake_quant_fork(x, spec, B, S, variants, imps, out=out)[0] is out and torch.equal(out, y)


def test_unsupported_raises():
    x, imps, variants = _inputs(torch.float32)
    for spec in (C.get_codec("mxfp4"), C.get_codec("channel_8"),
                 C.with_native_wire(C.get_codec("ref_int4_global"), "bf16")):
        with pytest.raises(ValueError):
            C.fake_quant_fork(x, spec, B, S, variants, imps)
    with pytest.raises(ValueError):       # 0 < k < S without an importance source
        C.fake_quant_fork(x, C.get_codec("int4_token"), B, S, [(None, 5)], imps)
