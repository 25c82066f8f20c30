"""The 16-bit wire formats (test_codec_wire16.py) on the HIP kernels of csrc/codec.hip - the W16 instantiations of
pack_kernel / unpack_kernel: GPU message bytes and decode against the CPU codec's over every native-row codec, wire,
activation dtype, ratio and selection, the edge rows of the CPU test through the kernels against the same independent
references, the argument checks and one graph replay."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import test_codec_wire16 as T
from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
# (B, S, H): a partial mask word; a chunk with idle lanes (H % 512 != 0) and rows that split a workgroup; the smallest row
SHAPES = [(2, 80, 512), (3, 33, 896), (1, 1, 32)]
RATIOS = [0.0, 0.5, 1.0]
INVALID_VALUE = 1               # hipErrorInvalidValue


def activations(B, S, H, dtype):
    """test_codec_digests.activations at any shape: integers / 37 in [-27, 27], one channel x 100."""
    i = torch.arange(B * S * H, dtype=torch.int64)
    x = (((i * 2654435761) % 2001 - 1000).double() / 37).float().reshape(B * S, H)
    x[:, 70 % H] *= 100
    return x.to(dtype)


def importance(B, S):
    """Dyadic importance [B, S] (integers / 2^e, window sums in [1, 2)): every partial sum is exact in fp32 and fp64,
    so top-rho cuts at the same k in the kernel's fp32 scan and the CPU's fp64 sums, inside the window at ratio 0.5."""
    e = (500 * S).bit_length() - 1
    j = torch.arange(B * S, dtype=torch.int64)
    return (((j * 40503) % 997 + 1).double() / 2 ** e).float().reshape(B, S)


@lru_cache(maxsize=None)
def cpu_ref(name, wire, dn, ratio, sel, shape):
    """(x, importance, spec, CPU message, layout, CPU fp32 decode); computed once, never modified."""
    B, S, H = shape
    x, imp, spec = activations(B, S, H, {"f32": F32, "bf16": BF16}[dn]), importance(B, S), T.spec_of(name, wire)
    msg, L = C.encode(x, spec, B, S, ratio, imp, selection=sel)
    return x, imp, spec, msg, L, C.decode(msg, spec, L, F32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("wire", T.WIRES)
@pytest.mark.parametrize("name", T.NATIVE_CODECS)
def test_gpu_equals_cpu(name, wire, shape):
    B, S, H = shape
    seen_k = set()
    for dn in ("f32", "bf16"):
        for ratio in RATIOS:
            for sel in ("ratio", "top_rho") if C.get_codec(name).uses_ratio else ("ratio",):
                x, imp, spec, m_cpu, L, y_cpu = cpu_ref(name, wire, dn, ratio, sel, shape)
                case = (dn, ratio, sel)
                m_dev, L2 = C.encode(x.to(DEV), spec, B, S, ratio, imp.to(DEV), selection=sel)
                assert L2 == L and L.hi_fmt == T.WIRES[wire], case
                m_gpu = m_dev.cpu()
                n = W.message_payload(m_cpu, L)
                assert W.message_payload(m_gpu, L) == n, case
                assert torch.equal(m_gpu[:n], m_cpu[:n]), (case, int((m_gpu[:n] != m_cpu[:n]).sum()))
                assert torch.isfinite(y_cpu).all()
                for src in (m_dev, m_cpu.to(DEV)):                      # unpack of the GPU's and of the CPU's message
                    y = C.decode(src, spec, L, F32).cpu()
                    assert torch.equal(T.bits_of_t(y), T.bits_of_t(y_cpu)), (case, int((y != y_cpu).sum()))
                    yb = C.decode(src, spec, L, BF16).cpu()
                    assert torch.equal(yb.view(torch.int16), y_cpu.to(BF16).view(torch.int16)), case
                assert torch.equal(T.bits_of_t(C.decode(m_gpu, spec, L, F32)), T.bits_of_t(y_cpu)), case
                seen_k.add(int(W.message_k(m_gpu, L).sum()))
    if C.get_codec(name).uses_ratio and S > 1:                           # all hi, mixed and all lo messages were seen
        assert 0 in seen_k and B * S in seen_k and len(seen_k) >= 3


# ---- the edge rows of the CPU test through the kernels ---------------------------------------------------------
def gpu_roundtrip(x, spec, B, S):
    msg, L = C.encode(x.to(DEV), spec, B, S)
    return msg, L, C.decode(msg, spec, L, F32).cpu()


@pytest.mark.parametrize("wire", ["bf16", "fp16"])
def test_elementwise_edge_rows(wire):
    """Ties of every kind, +-0, fp32 denormals, 65504 / 65520, the fp32 maximum, Inf and NaN: a truncating pack,
    flushed fp16 subnormals or a lost -0 fail the independent conversion."""
    x = T.edge_rows()
    spec = T.spec_of("passthrough", wire)
    m_dev, L, y = gpu_roundtrip(x, spec, T.ROWS_B, T.ROWS_S)
    m_gpu = m_dev.cpu()
    T.check_elementwise(wire, x, m_gpu, L, y)
    if wire == "fp16":
        T.check_fp16_promises(x, y)
    m_cpu, _ = C.encode(x, spec, T.ROWS_B, T.ROWS_S)
    nan = torch.isnan(x)                                                 # only a NaN's payload may differ
    assert torch.equal(m_gpu[:L.off_hi], m_cpu[:L.off_hi])
    assert np.array_equal(T.hi_rows_u16(m_gpu, L)[~nan.numpy()], T.hi_rows_u16(m_cpu, L)[~nan.numpy()])
    y_cpu = C.decode(m_cpu, spec, L, F32)
    assert torch.equal(T.bits_of_t(y)[~nan], T.bits_of_t(y_cpu)[~nan]) and torch.isnan(y[nan]).all()
    assert torch.equal(torch.isnan(C.decode(m_cpu.to(DEV), spec, L, F32).cpu()), nan)


@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_scaled_fp16_edge_rows(dn):
    """Row maxima at and one ulp below a power of two, at 2^-98 and below it (the clamp), at fp32 denormals and at the
    fp32 maximum, an all-zero row and rows with a NaN / an Inf (a max that drops a NaN would leave that row finite):
    p, the codes and the decode against the fp64 / integer reference.  bf16 activations: the same rows rounded."""
    x = T.s16_rows().to({"f32": F32, "bf16": BF16}[dn])
    spec = T.spec_of("passthrough", "fp16s")
    m_dev, L, y = gpu_roundtrip(x, spec, T.S16_B, T.S16_S)
    m_gpu = m_dev.cpu()
    T.check_f16s(x.float(), m_gpu, L, y)
    m_cpu, _ = C.encode(x, spec, T.S16_B, T.S16_S)
    y_cpu = C.decode(m_cpu, spec, L, F32)
    fin = torch.isfinite(x.float()).all(-1)                              # rows of a non-finite unit: finiteness only
    rb = L.row_bytes(L.hi_fmt)
    rows_gpu, rows_cpu = (m[L.off_hi:L.off_hi + x.shape[0] * rb].reshape(-1, rb) for m in (m_gpu, m_cpu))
    assert torch.equal(m_gpu[:L.off_hi], m_cpu[:L.off_hi]) and torch.equal(rows_gpu[fin], rows_cpu[fin])
    assert torch.equal(T.bits_of_t(y[fin]), T.bits_of_t(y_cpu[fin]))
    for dec in (y, C.decode(m_cpu.to(DEV), spec, L, F32).cpu(), C.decode(m_gpu, spec, L, F32)):
        assert not torch.isfinite(dec[~fin]).any()
    assert int((~fin).sum()) == (3 if dn == "f32" else 6)                # bf16: the three maxima near 2^128 round to Inf


@pytest.mark.parametrize("wire", ["fp16", "fp16s"])
def test_nonfinite_row_in_a_mixed_message(wire):
    """A NaN in a kept row and an Inf in a quantized row of int4_token: the kept row decodes as its wire defines (the
    whole row non-finite in fp16s, the NaN alone in fp16), the other rows as the CPU's."""
    B, S, H = 2, 40, 128
    x, imp = activations(B, S, H, F32), importance(B, S)
    spec = T.spec_of("int4_token", wire)
    lo = W.select_mask(imp, S // 2).reshape(-1)
    r_hi, r_lo = int((~lo).nonzero()[3]), int(lo.nonzero()[5])
    x[r_hi, 17], x[r_lo, 90] = float("nan"), float("inf")
    m_cpu, L = C.encode(x, spec, B, S, 0.5, imp)
    y_cpu = C.decode(m_cpu, spec, L, F32)
    m_dev, _ = C.encode(x.to(DEV), spec, B, S, 0.5, imp.to(DEV))
    y = C.decode(m_dev, spec, L, F32).cpu()
    clean = torch.ones(B * S, dtype=torch.bool)
    clean[[r_hi, r_lo]] = False
    assert torch.equal(T.bits_of_t(y[clean]), T.bits_of_t(y_cpu[clean])) and torch.isfinite(y[clean]).all()
    assert torch.equal(torch.isfinite(y), torch.isfinite(y_cpu))
    assert not torch.isfinite(y[r_lo]).any() and not torch.isfinite(y[r_hi, 17])
    assert bool(torch.isfinite(y[r_hi]).any()) == (wire == "fp16")


# ---- argument checks ---------------------------------------------------------------------------------------------
def test_rot_with_16bit_rows_is_rejected():
    """FMT_GRPR rows together with FMT_F16 / FMT_F16S rows: hipErrorInvalidValue, and nothing is launched (the
    message and the output keep their fill)."""
    from llm_inference_in_distributed_edge_networks_amd.ops import _native
    B, S, H = 2, 8, 128
    L = C.layout(W.with_plan(C.get_codec("rgroup_rot"), (4, 4)), B, S, H, 0, F32)
    gcb = sum(8 * b for b in L.plan)
    x = activations(B, S, H, F32).to(DEV)
    for fmt16 in (W.FMT_F16, W.FMT_F16S):
        for hi, lo in ((fmt16, W.FMT_GRPR), (W.FMT_GRPR, fmt16)):
            for entry, x_f32 in (("edge_pack", 1), ("edge_pack", 0), ("edge_unpack", 1), ("edge_unpack", 0)):
                msg = torch.full((1 << 16,), 0xAB, dtype=torch.uint8, device=DEV)   # room for any row format
                out = torch.full((B * S, H), 7.0, dtype=F32, device=DEV)
                buf = x if entry == "edge_pack" else out
                rc = getattr(_native.lib(), entry)(buf.data_ptr(), msg.data_ptr(), L.off_mask, L.off_scale, L.off_hi,
                                                   L.off_lo, -1, L.off_plan, B, S, H, 0, hi, lo, W.SC_NONE, 0, 0, 0,
                                                   gcb, x_f32, _native.stream())
                torch.cuda.synchronize()
                assert rc == INVALID_VALUE, (entry, hi, lo, rc)
                assert bool((msg == 0xAB).all()) and bool((out == 7.0).all())
    # the same call with rotated rows alone is accepted (the arguments above are otherwise valid)
    msg = torch.zeros(L.total, dtype=torch.uint8, device=DEV)
    msg[L.off_plan:L.off_plan + 2] = 4
    _native.call("edge_pack", x.data_ptr(), msg.data_ptr(), L.off_mask, L.off_scale, L.off_hi, L.off_lo, -1,
                 L.off_plan, B, S, H, 0, W.FMT_GRPR, W.FMT_GRPR, W.SC_NONE, 0, 0, 0, gcb, 1, _native.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("wire", T.WIRES)
def test_decode_into_both_dtypes(wire):
    """One message decoded into bf16 and into fp32 (given outputs and fresh ones): each the CPU's."""
    B, S, H = 3, 33, 896
    x, imp, spec, m_cpu, L, y_cpu = cpu_ref("int8_token_keep", wire, "f32", 0.5, "ratio", (B, S, H))
    m_dev, _ = C.encode(x.to(DEV), spec, B, S, 0.5, imp.to(DEV))
    for dtype in (F32, BF16):
        want = C.decode(m_cpu, spec, L, dtype)
        out = torch.full((B * S, H), 3.0, dtype=dtype, device=DEV)
        got = C.decode(m_dev, spec, L, dtype, out=out)
        assert got.data_ptr() == out.data_ptr() and got.dtype == dtype
        assert torch.equal(got.cpu(), want) and torch.equal(C.decode(m_dev, spec, L, dtype).cpu(), want)
    with pytest.raises(TypeError):
        C.decode(m_dev, spec, L, torch.float16)


# ---- graph replay ------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    """One encode / decode pair (int4_token with scaled fp16 kept rows: select, pack, unpack) captured by the
    project's GraphCache and replayed on other inputs, with the default queue settings."""
    from llm_inference_in_distributed_edge_networks_amd.utils.graphs import GraphCache
    B, S, H = 3, 33, 896
    spec = T.spec_of("int4_token", "fp16s")

    def step(x, imp):
        msg, L = C.encode(x, spec, B, S, 0.5, imp)
        return msg, C.decode(msg, spec, L, F32)

    cache = GraphCache(step)
    base, imp0 = activations(B, S, H, F32), importance(B, S)
    for i in range(4):                                                   # eager, capture + replay, replay, replay
        x = (base * (1 + i) + i).to(DEV)
        imp = imp0.roll(i, 1).contiguous().to(DEV)
        m_e, y_e = step(x, imp)
        m_g, y_g = cache(x, imp)
        assert torch.equal(m_g, m_e) and torch.equal(T.bits_of_t(y_g.cpu()), T.bits_of_t(y_e.cpu())), i
        m_cpu, L = C.encode(x.cpu(), spec, B, S, 0.5, imp.cpu())
        assert torch.equal(m_g.cpu(), m_cpu) and torch.equal(y_g.cpu(), C.decode(m_cpu, spec, L, F32))
    assert cache.graphs, "nothing was captured"
