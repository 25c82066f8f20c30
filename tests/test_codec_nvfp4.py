"""NVFP4 rows (codec/wire.py ``with_mx_elem`` "nvfp4": E2M1 codes, an E4M3 scale per 16 channels, one fp32 scale a row) on
the CPU oracle, against the definition worked out here: enumerated grids, fp64 / integer comparisons, and numpy float32
for the two steps the definition itself rounds once in fp32 (w = amb / g / 6 and x / d).  Channel 0 of every hard row is
2688 2^e, so g = 2^e exactly."""
import numpy as np
import pytest
import torch

from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

F32 = torch.float32
MX_CODECS = ["mxfp4", "mixed_mxfp4_mxfp8", "mxfp4_keep"]
EXPS = (0, -20, 100)
E4M3 = np.array([(m if e == 0 else 8 + m) * 2.0 ** (max(e, 1) - 10) for e in range(16) for m in range(8)][:127])
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
f32, up, down = np.float32, lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(0))
nv = lambda name: C.with_mx_elem(C.get_codec(name), "nvfp4")   # noqa: E731


def nearest(grid, y):
    """Index of the grid value nearest to min(|y|, max) (fp64: exact), a tie to the even index."""
    d = np.abs(grid - np.minimum(np.abs(np.asarray(y, dtype=np.float64)), grid[-1])[..., None])
    near = d == d.min(-1, keepdims=True)
    return np.where(near.sum(-1) == 2, (near & (np.arange(len(grid)) % 2 == 0)).argmax(-1), near.argmax(-1))


def expected(x, e):
    """(scale bytes [H/16], codes [H], values [H] fp64) of fp32 row x whose max-abs is 2688 2^e, by the definition."""
    blk = x.reshape(-1, 16)
    sb = nearest(E4M3, np.abs(blk).max(1) / f32(2.0 ** e) / f32(6))           # float32: the second division rounds once
    d = (E4M3[sb] * 2.0 ** e).astype(np.float32)                               # exact
    with np.errstate(all="ignore"):
        code = np.where((sb == 0)[:, None], 0, nearest(E2M1, blk / d[:, None]) | np.signbit(blk) << 3)
    return sb, code.reshape(-1), (np.where(code >= 8, -1.0, 1.0) * E2M1[code & 7] * d[:, None].astype(np.float64)).reshape(-1)


def scale_blocks():
    """[508, 16]: block 0 pins g (2688); block j >= 1 has one live channel 6 t_j: every E4M3 value, the midpoints of
    neighbours, an ulp either side of each, three tiny ones."""
    mid = ((E4M3[:-1] + E4M3[1:]) / 2).astype(np.float32)
    t = np.concatenate([E4M3[1:].astype(np.float32), mid, down(mid), up(mid), f32([2.0 ** -11, 2.0 ** -14, 2.0 ** -20])])
    x = np.zeros((len(t) + 1, 16), dtype=np.float32)
    x[0, 0] = 2688.0
    x[np.arange(1, len(t) + 1), np.arange(len(t)) % 16] = f32(6) * t
    return x


def code_blocks():
    """[40, 16]: blocks pinned by channel 0 at 6 s f (s: E4M3 values with mantissa bits, f: 1 and two factors that round
    back to s or on to its neighbour); the other 15 channels walk c s: the E2M1 grid, its midpoints +- an ulp, 0.1, both
    signs."""
    m = f32([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    c = np.concatenate([E2M1.astype(np.float32), m, down(m), up(m), f32([0.1])])
    c = np.concatenate([c, -c]).reshape(4, 15)
    pins = [(448.0, 1.0)] + [(s, f) for s in (1.125, 1.75, 3 * 2.0 ** -9) for f in (1.0, 33 / 32, 17 / 16)]
    return np.concatenate([np.concatenate([np.full((4, 1), 6 * s * f), c * f32(s)], 1) for s, f in pins]).astype(np.float32)


def hard_row(blocks, e, H=None, start=0):
    """Block 0, then the others from ``start`` on (all of them without H, else as many as H holds, wrapping), times 2^e."""
    rest = np.roll(blocks[1:], -start, 0)
    rest = rest if H is None else np.resize(rest, (H // 16 - 1, 16))
    return np.concatenate([blocks[:1], rest]).reshape(-1) * f32(2.0 ** e)


def unit_rows(H):
    """[6, H] Gaussian with: an all-zero row; a zero block; a denormal row; a NaN row; a -Inf row; one massive channel."""
    x = torch.randn(6, H, generator=torch.Generator().manual_seed(H))
    x[0], x[1, 16:32], x[3, 3], x[4, H - 2], x[5, H // 2] = 0.0, 0.0, float("nan"), float("-inf"), 3000.0
    x[2] *= 1e-40
    return x


def fields(raw, H):
    """(codes [n, H], scale bytes [n, H / 16], g [n]) of NVFP4 rows."""
    r = raw.numpy().reshape(-1, 9 * H // 16 + 4)
    return (np.stack([r[:, :H // 2] & 15, r[:, :H // 2] >> 4], -1).reshape(len(r), H), r[:, H // 2:-4],
            r[:, -4:].copy().view(np.float32)[:, 0])


def one_class(x):
    spec, H = nv("mxfp4"), x.shape[1]
    msg, L = C.encode(x, spec, 1, len(x), 0.0)
    assert L.hi_fmt == W.FMT_NVFP4 == 26 and L.row_bytes(26) == 9 * H // 16 + 4
    assert int(msg[28:32].view(torch.int32)) == 26 | 26 << 8
    return fields(msg[L.off_hi:L.off_hi + len(x) * L.row_bytes(26)], H), C.decode(msg, spec, L, F32).double().numpy()


@pytest.mark.parametrize("make", [scale_blocks, code_blocks])
def test_scale_bytes_and_codes(make):
    x = np.stack([hard_row(make(), e) for e in EXPS])
    (codes, sb, g), dec = one_class(torch.tensor(x))
    assert np.array_equal(g, f32(2.0) ** f32(EXPS))
    for i, e in enumerate(EXPS):
        want_sb, want, val = expected(x[i], e)
        assert np.array_equal(sb[i], want_sb) and np.array_equal(codes[i], want)
        assert np.array_equal(dec[i], val) and np.array_equal(np.signbit(dec[i]), want >= 8)
        q = np.abs(x[i].astype(np.float64)) / np.repeat(np.maximum(E4M3[want_sb], 2.0 ** -20) * 2.0 ** e, 16)
        if make is scale_blocks:                               # values -> their byte, midpoints -> the even byte, tiny -> 0
            assert np.array_equal(want_sb[:127], [126] + list(range(1, 127))) and not want_sb[505:].any() and len(want_sb) == 508
            assert np.array_equal(want_sb[127:253], np.arange(126) + np.arange(126) % 2) and want_sb[127] == 0
            assert not codes[i].reshape(-1, 16)[want_sb == 0].any()
        else:                                                # the band above 6 saturates; grid values keep their code
            assert ((q > 6) & (q <= 6.4)).sum() >= 12 and (want[q > 6] & 7 == 7).all()
            assert (want[q == 0] == [0, 8] * 10).all()       # the sign of zero is kept
            assert set(want_sb) == {126, 57, 58, 62, 63, 3} and ((want & 7)[q == 3] == 5).all()


def test_layout():
    H, B, S = 896, 2, 5
    rb = {W.FMT_F32: 4 * H, W.FMT_MXFP8: H + H // 32, W.FMT_NVFP4: 508}
    for name in MX_CODECS:
        for ratio in (0.0, 0.5, 1.0):
            L = C.layout(nv(name), B, S, H, W.num_lo(nv(name), ratio, S), F32)
            k = int(ratio * S) if nv(name).uses_ratio else 0
            assert L.lo_fmt == W.FMT_NVFP4 and C.message_bytes(nv(name), B, S, H, ratio, F32) == L.total == \
                32 + W._a16(B * L.mw * 4) + W._a16(B * (S - k) * rb[L.hi_fmt]) + W._a16(B * k * 508)
    for c in (0, 5, 15):                                     # -1 alone: g = 1 / 2688, its block's scale 448, code -6
        x = torch.zeros(1, 64)
        x[0, 16 + c] = -1.0
        (codes, sb, g), dec = one_class(x)
        assert codes[0, 16 + c] == 15 and codes.sum() == 15 and np.array_equal(sb[0], [0, 126, 0, 0])
        assert g[0] == f32(1) / f32(2688) and dec[0, 16 + c] == f32(-6) * (f32(448) * g[0])


def test_modifier():
    from llm_inference_in_distributed_edge_networks_amd.config import Params
    from llm_inference_in_distributed_edge_networks_amd.eval.sweep import SweepConfig
    from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig
    names, keep, rot = set(C.CODECS), nv("mxfp4_keep"), C.with_mx_rot(C.get_codec("mxfp4"), "h32")
    assert all(C.with_mx_elem(s, "fp4") is s for s in C.CODECS.values()) and W.FMT_NVFP4 not in W.MX_FORMATS
    for make, opt in ((lambda: nv("int8_token"), "mx_elem"), (lambda: C.with_native_wire(keep, "fp16"), "native_wire"),
                      (lambda: C.with_mx_elem(C.with_native_wire(C.get_codec("mxfp4_keep"), "fp16"), "nvfp4"), "mx_elem"),
                      (lambda: C.with_mx_rot(keep, "h32"), "mx_rot"), (lambda: C.with_mx_elem(rot, "nvfp4"), "mx_elem"),
                      (lambda: C.with_outliers(keep, "top8"), "outliers"), (lambda: C.with_row_rot(keep, "h128"), "row_rot"),
                      (lambda: Params.from_dict({"codec": "mxfp4", "mx_elem": "nvfp4", "mx_rot": "h32"}), "mx_rot")):
        with pytest.raises(ValueError, match=opt):
            make()
    assert not C.fork_supported(keep) and set(C.CODECS) == names
    msg, L = C.encode(torch.randn(10, 64), keep, 2, 5, 1.0)
    for other in (C.get_codec("mxfp4_keep"), C.with_mx_elem(C.get_codec("mxfp4_keep"), "e2m3")):
        for lay in (L, C.layout(other, 2, 5, 64, 5, F32)):  # the layout's formats; the header's word
            with pytest.raises(ValueError, match="format"):
                C.decode(msg, other, lay, F32)
    assert Params.from_dict({"codec": "mxfp4", "mx_elem": "nvfp4"}).mx_elem == SweepConfig([], [], [], mx_elem="nvfp4").mx_elem
    assert BoundaryConfig("mxfp4_keep", 0.5, mx_elem="nvfp4").spec_for(1, 64) == keep


def test_units():
    H, x = 128, unit_rows(128)
    (codes, sb, g), dec = one_class(x)
    assert g[0] == 0 and not codes[0].any() and not sb[0].any() and not dec[0].any()
    assert sb[1, 1] == 0 and not dec[1, 16:32].any() and sb[1, 0] and dec[1, :16].any()
    assert np.isfinite(dec[2]).all() and (np.abs(dec[2]) <= 2 * x[2].abs().max().item()).all()
    assert np.isnan(g[3]) and g[4] == np.inf and np.isnan(dec[3:5]).all() and np.isfinite(dec[[0, 1, 2, 5]]).all()
    assert not np.isin(sb, (0x7F, 0xFF)).any() and dec[5, H // 2] == f32(6) * (f32(448) * g[5])
    spec = nv("mxfp4")
    msg, L = C.encode(x, spec, 1, 6, 0.0)
    msg[L.off_hi + 5 * L.row_bytes(26) + H // 2 + 2] = 0x7F   # a received E4M3 NaN: its 16 channels, no others
    assert np.array_equal(np.nonzero(C.decode(msg, spec, L, F32)[5].isnan().numpy())[0], np.arange(32, 48))
