"""Rotated per-token int rows (``with_row_rot``) on the CPU oracle, against an explicit fp64 Sylvester matrix in numpy."""
import numpy as np
import pytest
import torch

from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W
from test_codec_outliers import B, CASES, IMP, NAMES, RATIO, S, same

F32, BF16 = torch.float32, torch.bfloat16
H128 = np.array([[(-1.0) ** bin(i & j).count("1") for j in range(128)] for i in range(128)])
BITS = {W.FMT_INT8R: 8, W.FMT_INT4R: 4, W.FMT_INT2R: 2}
NONFINITE = (3, 4, 5)


def hard_rows(H):
    """[10, H], integer-valued (the fp32 butterflies are exact): small values with one x1000 channel; spikes on the two
    sides of a block edge; all zero; one NaN; one Inf; 2^122 throughout (the butterflies overflow); |x| <= 2^10."""
    x = torch.randint(-8, 9, (10, H), generator=torch.Generator().manual_seed(H)).float()
    x[0, 70], x[1, 127], x[1, H - 128], x[2] = 3000.0, -5000.0, 7000.0, 0.0
    x[3, H // 2 + 5], x[4, 21], x[5] = float("nan"), float("inf"), 2.0 ** 122
    x[6:] = torch.randint(-1024, 1025, (4, H), generator=torch.Generator().manual_seed(H + 1)).float()
    return x


def ref_row(x, qmax, bits):
    """(scale, code bytes, decode) of one fp32 row in fp64, every fp32 operation of the codec rounded once."""
    y = (x.astype(np.float64).reshape(-1, 128) @ H128).astype(np.float32).astype(np.float64).reshape(-1) * 0.125
    am, s = np.abs(y).max(), np.float32(np.abs(y).max() / qmax)
    inv = np.float32(1.0 / np.float64(s)) if am > 0 else np.float32(0.0)
    q = np.clip(np.rint((y * np.float64(inv)).astype(np.float32).astype(np.float64)), -qmax, qmax)   # half to even
    q = np.nan_to_num(q).astype(np.int64)
    code = ((q & ((1 << bits) - 1)).reshape(-1, 8 // bits) << (bits * np.arange(8 // bits))).sum(1).astype(np.uint8)
    dec = ((q.reshape(-1, 128) @ H128.astype(np.int64)).reshape(-1) * np.float64(np.float32(s * np.float32(0.0625))))
    return s, code, dec.astype(np.float32)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,sel", CASES)
def test_cpu_codec_is_the_fp64_construction(name, sel, dtype):
    spec, H = C.with_row_rot(C.get_codec(name), "h128"), 256
    x = hard_rows(H).to(dtype)
    msg, L = C.encode(x, spec, B, S, RATIO, IMP, selection=sel)
    dec, xs = C.decode(msg, spec, L, dtype).float().numpy(), x.float().numpy()
    lo = W._words_to_mask(msg[L.off_mask:L.off_mask + 4 * B * L.mw].view(torch.int32).reshape(B, L.mw), S).reshape(-1)
    scales = msg[L.off_scale:L.off_scale + 4 * B * S].view(F32).numpy()
    assert int(msg[28:32].view(torch.int32)) == L.hi_fmt | L.lo_fmt << 8
    for fmt, qmax, rows, off in ((L.hi_fmt, spec.qmax_hi, ~lo, L.hi_offset(int(lo.sum()))),
                                 (L.lo_fmt, spec.qmax_lo, lo, L.off_lo)):
        for r in torch.nonzero(rows).flatten().tolist():
            if fmt not in BITS:                                      # a kept row: the activation's bits
                assert fmt == W.native_fmt(dtype) and same(dec[r], xs[r])
            else:
                with np.errstate(all="ignore"):
                    s, code, want = ref_row(xs[r], qmax, BITS[fmt])
                assert same(scales[r], s) and same(dec[r], torch.from_numpy(want).to(dtype).float().numpy()), r
                assert np.isfinite(dec[r]).sum() == (0 if r in NONFINITE else H), r
                assert r in NONFINITE or np.array_equal(msg[off:off + L.row_bytes(fmt)].numpy(), code), (r, "codes")
            off += L.row_bytes(fmt)


def test_spec_rules():
    from dataclasses import replace
    from llm_inference_in_distributed_edge_networks_amd.config import Params
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig
    get, rot = C.get_codec, lambda n: C.with_row_rot(C.get_codec(n), "h128")
    r4, mx = rot("int4_token"), replace(get("mxfp4"), row_rot=128)
    assert len(C.CODECS) == 18
    for n in NAMES:
        plain, r = get(n), rot(n)
        assert C.with_row_rot(plain, "none") is plain and not C.fork_supported(r)
        for ratio in (0.0, 0.4, 1.0):
            Lp, Lr = (C.layout(s, B, S, 896, W.num_lo(plain, ratio, S), F32) for s in (plain, r))
            assert (Lr.hi_fmt, Lr.lo_fmt) == tuple(W.ROW_ROT_TWIN.get(f, f) for f in (Lp.hi_fmt, Lp.lo_fmt))
            assert (Lr.off_hi, Lr.off_lo, Lr.total) == (Lp.off_hi, Lp.off_lo, Lp.total)
        with pytest.raises(ValueError, match="128"):
            C.layout(r, B, S, 96, 2, F32)
    with pytest.raises(ValueError, match="fake_quant_fork"):
        C.fake_quant_fork(torch.zeros(B * S, 128), r4, B, S, [(None, 0)])
    for make in ([lambda n=n: rot(n) for n in C.CODECS if n not in NAMES] +
                 [lambda: C.with_row_rot(get("int4_token"), "h64"), lambda: C.with_native_wire(r4, "fp16"),
                  lambda: C.with_row_rot(C.with_native_wire(get("int4_token"), "bf16"), "h128"),
                  lambda: C.with_outliers(r4, "top8"), lambda: C.with_row_rot(C.with_outliers(get("int4_token"), "top8"), "h128"),
                  lambda: C.with_mx_elem(mx, "e2m3"), lambda: C.with_row_rot(C.with_mx_elem(get("mxfp4_keep"), "e2m3"), "h128"),
                  lambda: C.with_mx_rot(mx, "h32"), lambda: C.with_row_rot(C.with_mx_rot(get("mxfp4"), "h32"), "h128"),
                  lambda: Params.from_dict({"codec": "ref_int4_global", "row_rot": "h128"}),
                  lambda: Params.from_dict({"codec": "int4_token", "row_rot": "h128", "outliers": "top8"})]):
        with pytest.raises(ValueError, match="row_rot"):
            make()
    assert Params.from_dict({}).row_rot == BoundaryConfig().row_rot == "none"
    assert BoundaryConfig("int4_token", 0.5, row_rot="h128").spec_for(1, 128) == r4
    x, plain = torch.ones(B * S, 128), get("int4_token")               # a foreign message is refused, both ways
    (m_rot, L_rot), (m_plain, L_plain) = C.encode(x, r4, B, S, RATIO, IMP), C.encode(x, plain, B, S, RATIO, IMP)
    for m, spec, lay in ((m_rot, plain, L_plain), (m_plain, r4, L_rot), (m_rot, plain, L_rot), (m_plain, r4, L_plain)):
        with pytest.raises(ValueError, match="format"):
            C.decode(m, spec, lay, F32)


def test_one_massive_channel_no_longer_sets_the_int8_step():
    x = torch.randn(256, 896, generator=torch.Generator().manual_seed(0)) * (1 + 999 * (torch.arange(896) == 70))
    mse = [float((C.fake_quant(x, s, 1, 256, 1.0)[0] - x).square().mean())
           for s in (C.get_codec("int8_token"), C.with_row_rot(C.get_codec("int8_token"), "h128"))]
    print(f"int8_token MSE {mse[0]:.4g}, @h128 {mse[1]:.4g}, ratio {mse[0] / mse[1]:.1f}")
    assert mse[1] < mse[0]
