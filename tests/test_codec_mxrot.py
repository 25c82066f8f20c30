"""Rotated MX rows (codec/wire.py ``with_mx_rot``) on the CPU oracle, against an explicit +-1 Hadamard matrix in fp64."""
from dataclasses import replace

import pytest
import torch

from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

F32 = torch.float32
ELEMS = {"fp4": ("mxfp4", "fp4"), "e2m3": ("mxfp4", "e2m3"), "e3m2": ("mxfp4", "e3m2"), "e4m3": ("mxfp8", "fp4")}
MX_CODECS = ["mxfp4", "mxfp8", "mixed_mxfp4_mxfp8", "mxfp4_keep"]
H2 = torch.tensor([[1.0, 1.0], [1.0, -1.0]], dtype=torch.float64)
H32 = torch.kron(torch.kron(torch.kron(H2, H2), torch.kron(H2, H2)), H2)     # y_i = sum_j (-1)^popcount(i & j) x_j


def unit_rows(H):
    """[6, H] of small integers; block 0 of the rows: one-hot 4, zero, a NaN, an Inf, all 2^125, denormals k 1e-39."""
    x = torch.randint(-8, 9, (6, H), generator=torch.Generator().manual_seed(H)).float()
    x[:, :32] = 0.0
    x[0, 5], x[2, 3], x[3, 7] = 4.0, float("nan"), float("-inf")
    x[4, :32], x[5, :32] = 2.0 ** 125, torch.arange(-16, 16) * 1e-39
    return x


@pytest.mark.parametrize("elem", list(ELEMS))
def test_round_trip_is_h32_q_h32_in_fp64(elem):
    plain = C.with_mx_elem(C.get_codec(ELEMS[elem][0]), ELEMS[elem][1])
    x = torch.randint(-8, 9, (4, 96), generator=torch.Generator().manual_seed(1)).float()
    x[:, 40] *= 100                                          # integers: every fp32 butterfly is exact
    y = (x.double().reshape(4, 3, 32) @ H32 / 4).reshape(4, 96).float()
    q = C.fake_quant(y, plain, 1, 4)[0]                      # Q: the plain round trip of the same element type
    got = C.fake_quant(x, C.with_mx_rot(plain, "h32"), 1, 4)[0]
    assert torch.equal(got.double(), (q.double().reshape(4, 3, 32) @ H32 / 8).reshape(4, 96))


@pytest.mark.parametrize("elem", list(ELEMS))
def test_units(elem):
    plain = C.with_mx_elem(C.get_codec(ELEMS[elem][0]), ELEMS[elem][1])
    H, x, rot = 64, unit_rows(64), C.with_mx_rot(plain, "h32")
    msg, L = C.encode(x, rot, 1, 6)
    fmt, rb = C.layout(plain, 1, 6, H, 0, F32).hi_fmt, L.row_bytes(L.hi_fmt)
    raw, dec = msg[L.off_hi:L.off_hi + 6 * rb].reshape(6, rb), C.decode(msg, rot, L, F32)
    assert L.hi_fmt == W.MX_ROT_TWIN[fmt] and rb == W.ROW_FORMATS[fmt].row_bytes(H, None)
    assert raw[:, rb - 2].tolist()[1:5] == [0, 255, 255, 255]            # block 0's scale byte: zero, NaN, Inf, overflow
    codes = W._mx_unpack(raw[0], fmt, 1, H)[0, :32]
    assert (codes.abs() == codes[0].abs()).all() and codes[0] != 0       # a one-hot: 32 codes of one magnitude
    assert torch.equal(dec[:2, :32], x[:2, :32])                         # the one-hot and the zero block: exact
    assert dec[2:5, :32].isnan().all() and dec[:, 32:].isfinite().all() and dec[5].isfinite().all()


@pytest.mark.parametrize("name", MX_CODECS)
def test_wire_bytes_header_and_foreign_messages(name):
    plain, B, S, H = C.get_codec(name), 2, 5, 896
    rot = C.with_mx_rot(plain, "h32")
    assert C.with_mx_rot(plain, "none") is plain and not C.fork_supported(rot)
    for ratio in (0.0, 0.4, 1.0):
        Lp, Lr = (C.layout(s, B, S, H, W.num_lo(s, ratio, S), F32) for s in (plain, rot))
        twins = {k: W.MX_ROT_TWIN.get(getattr(Lp, k), getattr(Lp, k)) for k in ("hi_fmt", "lo_fmt")}
        assert Lr == replace(Lp, **twins) != Lp
        assert C.message_bytes(rot, B, S, H, ratio, F32) == C.message_bytes(plain, B, S, H, ratio, F32) == Lp.total
    x, imp = torch.randn(B * S, 64), torch.rand(B, S)
    (msg, L), (m_plain, L_plain) = C.encode(x, rot, B, S, 0.4, imp), C.encode(x, plain, B, S, 0.4, imp)
    assert int(msg[28:32].view(torch.int32)) == L.hi_fmt | L.lo_fmt << 8
    for m, spec, lay in ((msg, plain, L_plain), (m_plain, rot, L), (msg, plain, L), (m_plain, rot, L_plain)):
        with pytest.raises(ValueError, match="format"):                  # a rotated message under the plain spec and back
            C.decode(m, spec, lay, F32)


def test_modifier_refusals_and_defaults():
    from llm_inference_in_distributed_edge_networks_amd.config import Params
    from llm_inference_in_distributed_edge_networks_amd.eval.sweep import SweepConfig
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig
    keep = C.with_mx_rot(C.get_codec("mxfp4_keep"), "h32")
    for make in (lambda: C.with_mx_rot(C.get_codec("int8_token"), "h32"), lambda: C.with_mx_rot(keep, "h64"),
                 lambda: C.with_native_wire(keep, "fp16"),
                 lambda: C.with_mx_rot(C.with_native_wire(C.get_codec("mxfp4_keep"), "fp16"), "h32"),
                 lambda: Params.from_dict({"codec": "rgroup_rot", "mx_rot": "h32"})):
        with pytest.raises(ValueError, match="mx_rot"):
            make()
    assert Params.from_dict({}).mx_rot == BoundaryConfig().mx_rot == SweepConfig([], [], []).mx_rot == "none"
    assert BoundaryConfig("mxfp4_keep", 0.5, mx_rot="h32").spec_for(1, 64) == keep and len(C.CODECS) == 18
