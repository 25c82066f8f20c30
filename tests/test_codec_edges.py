"""Boundary codec on the inputs a Gaussian tensor almost never holds: values exactly on a rounding boundary (and one
ulp off it), values that saturate, units (row, group, block, window, channel) whose max-abs is 0, scales at both ends
of the exponent range, NaN and Inf.

Every expectation here comes from an independent reference in fp64 / fp32 numpy, never from a second call into
``codec/wire.py``:

* integer grids: with a unit's scale pinned to a power of two, x / s is exact in fp64 and the expected code is its
  round-half-even (``numpy.rint``, checked against Python's ``round`` of the exact ``Fraction`` below), clamped;
* E2M1 / E4M3: the finite grid enumerated from the format definition (sign, exponent, mantissa, subnormals); the
  expected decode of x in a block of scale X = 2^(floor(log2 amax) - emax) is X times the grid point nearest to
  x / X, ties to the even code, saturating at the largest grid point;
* the window / channel formulas of the reference (divide, then multiply) in numpy fp32 arithmetic, step by step;
* Hadamard rows: the fp64 transform H64 x / 8.

The case builders (``*_case`` functions, cached) are shared with ``test_codec_edges_gpu.py``, which runs the same
cases on the HIP kernels against the CPU message bytes, the CPU decode and the same independent checks.
"""
from dataclasses import dataclass, field
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest
import torch

from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

F32, BF16 = torch.float32, torch.bfloat16
E_WINDOWS = (0, -20, 60)             # window b of a tie case pins its scales to 2^E_WINDOWS[b]
X_WINDOWS = (0, -30, 40)             # window b of an MX grid case has block scale 2^X_WINDOWS[b]
INT_FMTS = (W.FMT_INT8, W.FMT_INT4, W.FMT_INT2)
# (B, S, H): S = 64 fills both mask words, S = 37 leaves the last one partial; H = 576 is 9 groups (the second lane
# chunk half used), 896 the model's width
SHAPES = [(3, 64, 64), (3, 64, 128), (3, 64, 576), (3, 64, 896), (3, 37, 576)]
MX_SHAPES = SHAPES + [(3, 64, 96), (3, 37, 96)]


# ---- independent references -------------------------------------------------------------------------------------
def minifloat_grid(ebits, mbits, bias, drop_top=0):
    """Non-negative finite values of a sign / exponent / mantissa format in code order (exponent field 0:
    subnormals m / 2^mbits * 2^(1 - bias)); ``drop_top`` codes at the top are not numbers (E4M3: one NaN)."""
    g = [(m / 2 ** mbits) * 2.0 ** (1 - bias) if e == 0 else (1 + m / 2 ** mbits) * 2.0 ** (e - bias)
         for e in range(2 ** ebits) for m in range(2 ** mbits)]
    return np.array(g[:len(g) - drop_top])


E2M1 = minifloat_grid(2, 1, 1)
E4M3 = minifloat_grid(4, 3, 7, drop_top=1)
MX_GRID = {W.FMT_MXFP4: (E2M1, 2), W.FMT_MXFP8: (E4M3, 8)}      # grid, emax


def grid_index(y, grid):
    """Index of the grid point nearest to |y| (fp64, exact inputs): ties to the even index, saturating."""
    a = np.abs(y)
    hi = np.clip(np.searchsorted(grid, a, side="left"), 1, len(grid) - 1)
    lo = hi - 1
    dlo, dhi = a - grid[lo], grid[hi] - a
    idx = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    return np.where(a >= grid[-1], len(grid) - 1, idx)


def mx_reference(x64, fmt):
    """OCP MX rows [n, H] (fp64 copies of fp32 values) -> (decode fp64, E8M0 bytes [n, H/32])."""
    grid, emax = MX_GRID[fmt]
    n, H = x64.shape
    blk = x64.reshape(n, H // 32, 32)
    am = np.abs(blk).max(-1)
    _, ex = np.frexp(am)                                      # am = m 2^ex, m in [0.5, 1)
    e = np.where(am >= 2.0 ** -126, ex - 1, -127)             # zero / denormal max-abs: exponent field 0
    sb = np.clip(e - emax + 127, 0, 254)
    X = 2.0 ** (sb - 127.0)
    y = blk / X[..., None]
    dec = np.copysign(grid[grid_index(y, grid)], blk) * X[..., None]
    return dec.reshape(n, H), sb


H64 = np.array([[-1.0 if bin(a & b).count("1") & 1 else 1.0 for b in range(64)] for a in range(64)])   # Sylvester


def hadamard_groups(g64):
    """H64 x / 8 of every 64-channel group [..., 64] in fp64 (H64[i, j] = (-1)^popcount(i & j))."""
    return g64 @ H64 / 8.0


def qmax_of_bits(b):
    return (1 << (b - 1)) - 1


# ---- selection, formats, message sections -----------------------------------------------------------------------
def importance(B, S):
    """Distinct values per window (7 is coprime to 64 and 37), so the k least important tokens need no tie rule."""
    j = torch.arange(S)
    return torch.stack([((j * 7 + 3 * b) % S).float() / S for b in range(B)])


def lo_mask(spec, ratio, imp):
    B, S = imp.shape
    k = int(ratio * S) if spec.uses_ratio else 0
    lo = np.zeros((B, S), dtype=bool)
    order = np.argsort(imp.numpy(), axis=1, kind="stable")
    for b in range(B):
        lo[b, order[b, :k]] = True
    return lo


def all_widths(H):
    return tuple(W.GROUP_BITS[g % len(W.GROUP_BITS)] for g in range(H // 64))


def spec_of(name, H, plan=None):
    spec = C.get_codec(name)
    return W.with_plan(spec, plan or all_widths(H)) if W.needs_plan(spec) else spec


def row_formats(spec, lo, dtype):
    """Per row [B * S]: the row format and the integer formats' qmax."""
    nf = W.native_fmt(dtype)
    hi_f = nf if spec.hi_fmt == W.NATIVE else spec.hi_fmt
    lo_f = nf if spec.lo_fmt == W.NATIVE else spec.lo_fmt
    l = lo.reshape(-1)
    return np.where(l, lo_f, hi_f), np.where(l, spec.qmax_lo, spec.qmax_hi)


def scale_section(msg, L, spec):
    n = {W.SC_TOKEN: L.B * L.S, W.SC_WINDOW: L.B, W.SC_CHANNEL: L.B * L.H}.get(spec.scale_mode, 0)
    return msg[L.off_scale:L.off_scale + 4 * n].clone().view(torch.float32).numpy()


def uniform_rows(msg, L):
    """The rows [B * S, row bytes] of a message whose rows all have the hi format (k = 0), in token order."""
    assert L.k == 0 and not L.kvar
    rb = L.row_bytes(L.hi_fmt)
    return msg[L.off_hi:L.off_hi + L.B * L.S * rb].reshape(L.B * L.S, rb)


def inline_scales(msg, L):
    """Scales stored inside uniform rows: fp32 [B * S, G] of head-group rows, E8M0 bytes [B * S, H / 32] of MX rows."""
    r = uniform_rows(msg, L)
    if L.hi_fmt in W.GRP_FORMATS:
        cb = sum(8 * b for b in L.plan)
        return r[:, cb:].contiguous().view(torch.float32).numpy()
    nc = L.H // 2 if L.hi_fmt == W.FMT_MXFP4 else L.H
    return r[:, nc:].numpy().astype(np.int64)


def window_bytes(L, spec, b):
    """bool [message bytes]: the scale and row bytes that belong to window b (fixed-k layout)."""
    m = np.zeros(L.total, dtype=bool)
    per = 4 * {W.SC_TOKEN: L.S, W.SC_WINDOW: 1, W.SC_CHANNEL: L.H}.get(spec.scale_mode, 0)
    hi, lo = (L.S - L.k) * L.row_bytes(L.hi_fmt), L.k * L.row_bytes(L.lo_fmt)
    m[L.off_scale + b * per:L.off_scale + (b + 1) * per] = True
    m[L.off_hi + b * hi:L.off_hi + (b + 1) * hi] = True
    m[L.off_lo + b * lo:L.off_lo + (b + 1) * lo] = True
    return m


# ---- input builders ---------------------------------------------------------------------------------------------
def units(T, D, pins, U):
    """[n, U] values and ulp offsets: unit i holds ``pins[i]`` at position i % U and U - 1 consecutive entries of the
    list (T, D), starting where unit i - 1 stopped, so a few units cover the whole list."""
    n = len(pins)
    idx = (np.arange(n)[:, None] * (U - 1) + np.arange(U - 1)[None, :]) % len(T)
    cols = np.arange(U)[None, :]
    p = (np.arange(n) % U)[:, None]
    src = np.minimum(np.where(cols > p, cols - 1, cols), U - 2)
    Tu, Du = np.take_along_axis(T[idx], src, 1), np.take_along_axis(D[idx], src, 1)
    Tu[cols == p], Du[cols == p] = pins, 0
    return Tu, Du


def realize(T, D, dtype):
    """fp64 values -> tensor of ``dtype`` (round to nearest), then D ulps of that dtype away from zero (D = -1:
    towards zero); zeros keep their sign and stay zero."""
    v = torch.from_numpy(np.ascontiguousarray(T)).to(dtype)
    bits = v.view(torch.int32 if dtype == F32 else torch.int16)
    d = torch.from_numpy(np.ascontiguousarray(D)).to(bits.dtype) * (v != 0).to(bits.dtype)
    return (bits + d).view(dtype)


def with_ulps(t, extra=()):
    """The list (T, D): every t exactly, one ulp above and one below in magnitude; ``extra`` values exactly."""
    t, extra = np.asarray(t, dtype=np.float64), np.asarray(extra, dtype=np.float64)
    z = np.zeros(len(t), dtype=np.int64)
    return np.concatenate([t, t, t, extra]), np.concatenate([z, z + 1, z - 1, np.zeros(len(extra), dtype=np.int64)])


@lru_cache(maxsize=None)
def tie_list(qmax):
    """Every (k + 0.5) for k in [-qmax, qmax - 1] (in units of the step), each also at +-1 ulp, and +-0."""
    return with_ulps(np.arange(-qmax, qmax) + 0.5, [0.0, -0.0])


def tie_units(qunit, U):
    """Tie units [n, U] in units of the step for per-unit qmax ``qunit``: pin +-qmax, the rest from tie_list."""
    n = len(qunit)
    T, D = np.zeros((n, U)), np.zeros((n, U), dtype=np.int64)
    for q in np.unique(qunit):
        i = np.nonzero(qunit == q)[0]
        T[i], D[i] = units(*tie_list(int(q)), np.where(i % 2 == 0, float(q), -float(q)), U)
    return T, D


@lru_cache(maxsize=None)
def mx_list(fmt):
    """Every midpoint between adjacent grid points at both signs, each also at +-1 ulp; +-0; fp4: +-0.1 (rounds to a
    signed zero); fp8: +-500 (above 448: clamps) and +-0.0009 (below half the smallest subnormal 2^-9)."""
    grid = MX_GRID[fmt][0]
    mid = (grid[:-1] + grid[1:]) / 2
    extra = [0.0, -0.0, 0.1, -0.1] if fmt == W.FMT_MXFP4 else [0.0, -0.0, 500.0, -500.0, 0.0009, -0.0009]
    return with_ulps(np.concatenate([mid, -mid]), extra)


@dataclass
class Case:
    spec: object
    B: int
    S: int
    H: int
    ratio: float
    imp: torch.Tensor
    x: torch.Tensor                      # [B * S, H] activations (fp32 or bf16)
    lo: np.ndarray                       # bool [B, S], from the independent selection
    info: dict = field(default_factory=dict)

    @property
    def x64(self):
        return self.x.double().numpy()

    def cpu(self):
        """(message, layout, fp32 decode) of the CPU oracle."""
        msg, L = C.encode(self.x, self.spec, self.B, self.S, self.ratio, self.imp)
        return msg, L, C.decode(msg, self.spec, L, F32)


def new_case(name, ratio, B, S, H, x, plan=None, **info):
    spec = spec_of(name, H, plan)
    imp = importance(B, S)
    return Case(spec, B, S, H, ratio, imp, x, lo_mask(spec, ratio, imp), info)


def same(y, exp64):
    """fp32 decode == fp64 expectation, value for value."""
    got = y.double().numpy()
    bad = got != exp64
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} differ; first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[bad][0]!r} != {exp64[bad][0]!r}"


# ---- family 1: ties with a pinned scale ----------------------------------------------------------------------------
TIE_CODECS = ["int8_token", "int4_token", "mixed_int4_int8", "mixed_int2_int8", "int8_token_keep", "rgroup",
              "mixed_rgroup_int8"]


def tie_params():
    return [(n, r, *shp) for n in TIE_CODECS for r in ((0.0, 0.5, 1.0) if C.get_codec(n).uses_ratio else (0.0,))
            for shp in SHAPES]


@lru_cache(maxsize=None)
def tie_case(name, ratio, B, S, H, dtype=F32):
    """Every unit's max-abs is qmax 2^e (e by window: E_WINDOWS), so its scale is 2^e, 1 / s and x / s are exact, and
    the unit's other elements walk through every half-way point of its grid, +-1 ulp, and +-0.  Native rows hold the
    int8 list.  info: per element the step and qmax (0: native)."""
    spec = spec_of(name, H)
    lo = lo_mask(spec, ratio, importance(B, S))
    fmt, qrow = row_formats(spec, lo, dtype)
    step = np.repeat(2.0 ** np.array(E_WINDOWS[:B], dtype=np.float64), S)[:, None] * np.ones((1, H))
    q = np.zeros((B * S, H), dtype=np.int64)
    T, D = tie_units(np.where(np.isin(fmt, INT_FMTS), qrow, 127), H)
    q[np.isin(fmt, INT_FMTS)] = qrow[np.isin(fmt, INT_FMTS)][:, None]
    grp = np.nonzero(np.isin(fmt, W.GRP_FORMATS))[0]
    if len(grp):
        qg = np.array([qmax_of_bits(b) for b in spec.plan])
        Tg, Dg = tie_units(np.tile(qg, len(grp)), 64)
        T[grp], D[grp] = Tg.reshape(len(grp), H), Dg.reshape(len(grp), H)
        q[grp] = np.repeat(qg, 64)[None, :]
    return new_case(name, ratio, B, S, H, realize(T * step, D, dtype), step=step, q=q, fmt=fmt)


def tie_expect(case):
    x, step, q = case.x64, case.info["step"], case.info["q"]
    code = np.clip(np.rint(x / step), -q, q)                 # x / 2^e is exact; rint is round-half-even
    return np.where(q > 0, code * step, x)


def check_ties(case, msg, L, y):
    same(y, tie_expect(case))
    fmt, step = case.info["fmt"], case.info["step"]
    if case.spec.scale_mode == W.SC_TOKEN:                    # token scale 2^e; 0 for rows that carry their own
        exp = np.where(np.isin(fmt, INT_FMTS), step[:, 0], 0.0)
        assert np.array_equal(scale_section(msg, L, case.spec).astype(np.float64), exp)
    if case.spec.name == "rgroup":
        assert np.array_equal(inline_scales(msg, L).astype(np.float64), step[:, ::64])


def test_half_even_table():
    """numpy.rint on the exact quotient is the literal half-even table: Python's round of the exact Fraction."""
    for qmax in (1, 3, 7, 15, 31, 127):
        T, _ = tie_list(qmax)
        for e in E_WINDOWS:
            for t in T[:2 * qmax]:
                x = float(np.float32(t * 2.0 ** e))
                assert x == t * 2.0 ** e
                assert np.rint(x / 2.0 ** e) == round(Fraction(x) / Fraction(2) ** e), (qmax, e, t)
    assert [int(np.rint(v)) for v in (-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 6.5)] == [-2, -2, 0, 0, 2, 2, 6]


def test_grids_from_definition():
    assert E2M1.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert len(E4M3) == 127 and E4M3[-1] == 448.0 and E4M3[1] == 2.0 ** -9 and E4M3[8] == 2.0 ** -6
    assert (np.diff(E4M3) > 0).all()
    # ties go to the even code, values past the largest grid point saturate
    assert grid_index(np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.9]), E2M1).tolist() == [0, 2, 2, 4, 4, 6, 6, 7]
    assert E4M3[grid_index(np.array([432.0, 500.0, 2.0 ** -10, 3 * 2.0 ** -10]), E4M3)].tolist() == \
        [448.0, 448.0, 0.0, 2.0 ** -8]


def test_tie_cases_cover_every_tie():
    """The builder reaches every half-way point of every width, at both neighbours, in every window."""
    case = tie_case("rgroup", 0.0, 3, 37, 576)
    x, step, q = case.x64, case.info["step"], case.info["q"]
    for b in range(3):
        rows = slice(b * 37, b * 37 + 37)
        for g, bits in enumerate(case.spec.plan):
            v = (x[rows, 64 * g:64 * g + 64] / step[rows, 64 * g:64 * g + 64]).reshape(-1)
            qm = qmax_of_bits(bits)
            assert np.abs(v).max() == qm
            for k in range(-qm, qm):
                near = v[np.abs(v - (k + 0.5)) < 1e-4]
                assert (near == k + 0.5).any() and (near < k + 0.5).any() and (near > k + 0.5).any(), (b, bits, k)
    case = tie_case("mixed_int4_int8", 0.5, 3, 64, 64)
    assert set(np.unique(case.info["q"])) == {7, 127} and case.lo.sum() == 3 * 32


@pytest.mark.parametrize("name,ratio,B,S,H", tie_params())
def test_ties(name, ratio, B, S, H):
    case = tie_case(name, ratio, B, S, H)
    check_ties(case, *case.cpu())


@pytest.mark.parametrize("name,ratio", [("int8_token", 0.0), ("mixed_int4_int8", 0.5), ("mixed_int2_int8", 0.5),
                                        ("int8_token_keep", 0.5), ("mixed_rgroup_int8", 0.5), ("rgroup", 0.0)])
def test_ties_bf16(name, ratio):
    case = tie_case(name, ratio, 3, 37, 576, BF16)
    check_ties(case, *case.cpu())


# ---- family 2: window and channel formulas ------------------------------------------------------------------------
FORMULA_CODECS = ["ref_int4_global", "channel_8", "channel_4", "channel_1_max"]
FORMULA_MAXIMA = {"pow2": None, "npo2": (1.0, 3.3)}           # pow2: qmax 2^e per window (E_WINDOWS)


def formula_params():
    return [(n, r, v, *shp) for n in FORMULA_CODECS for r in ((0.5, 1.0) if n == "ref_int4_global" else (0.0,))
            for v in FORMULA_MAXIMA for shp in SHAPES]


@lru_cache(maxsize=None)
def formula_case(name, ratio, variant, B, S, H, dtype=F32):
    """The tie lists under the reference's divide-then-multiply formulas: the window max (over the lo rows) or every
    channel max is qmax 2^e, or 1.0 / 3.3 (no power of two: x / m * qmax rounds twice, the tie values land next to
    the ties).  Units are token rows (window mode: every row holds the window max) or channel columns."""
    spec = C.get_codec(name)
    q = spec.qmax_lo
    if variant == "npo2":
        B = 2
        maxima = [float(torch.tensor(m).to(dtype)) for m in FORMULA_MAXIMA["npo2"]]
    else:
        maxima = [q * 2.0 ** e for e in E_WINDOWS[:B]]
    xs = []
    for b, m in enumerate(maxima):
        if spec.scale_mode == W.SC_WINDOW:
            T, D = tie_units(np.full(S, q), H)
        else:
            T, D = (a.T for a in tie_units(np.full(H, q), S))
        xs.append(realize(T * (m / q), D, dtype))
    return new_case(name, ratio, B, S, H, torch.cat(xs), maxima=maxima)


def formula_expect(case):
    """(decode fp32, scale section fp32) by the reference's formulas in fp32 arithmetic, one operation at a time."""
    spec, B, S, H = case.spec, case.B, case.S, case.H
    x = case.x.float().numpy().reshape(B, S, H)
    q = np.float32(spec.qmax_lo)
    out = x.copy()
    if spec.scale_mode == W.SC_WINDOW:
        scales = np.zeros(B, dtype=np.float32)
        for b in range(B):
            rows = x[b][case.lo[b]]
            if not len(rows):
                continue
            m = scales[b] = np.abs(rows).max()
            code = np.rint(np.clip(rows / m * q, -(q + 1), q))
            out[b][case.lo[b]] = code / q * m
        return out, scales
    sc = np.abs(x).max(1)                                    # [B, H]
    safe = np.where(sc > 0, sc, np.float32(1))[:, None, :]
    if spec.qmax_lo == 1:
        out = np.clip(np.rint(x / safe), -1, 1) * sc[:, None, :]
    else:
        out = np.rint(x / safe * q) * sc[:, None, :] / q
    return np.where(sc[:, None, :] > 0, out, np.float32(0)), sc.reshape(-1)


def ref_q1_torch(case):
    """The reference's Q1 in torch, window by window (as tests/test_f32_gpu.py::test_codec_fp32_bitexact_vs_cpu)."""
    x = case.x.float().view(case.B, case.S, case.H).clone()
    for b in range(case.B):
        idx = torch.from_numpy(np.nonzero(case.lo[b])[0])
        if len(idx):
            m = x[b][idx].abs().max()
            x[b][idx] = torch.round(torch.clamp(x[b][idx] / m * 7.0, -8.0, 7.0)) / 7.0 * m
    return x.view(-1, case.H)


def check_formula(case, msg, L, y):
    dec, scales = formula_expect(case)
    assert dec.dtype == np.float32 and scales.dtype == np.float32
    assert np.array_equal(scale_section(msg, L, case.spec), scales)
    same(y, dec.reshape(-1, case.H).astype(np.float64))
    if case.spec.name == "ref_int4_global":
        assert torch.equal(y, ref_q1_torch(case))
    assert np.array_equal(scales.reshape(case.B, -1).max(1).astype(np.float64), np.array(case.info["maxima"]))


@pytest.mark.parametrize("name,ratio,variant,B,S,H", formula_params())
def test_formulas(name, ratio, variant, B, S, H):
    case = formula_case(name, ratio, variant, B, S, H)
    check_formula(case, *case.cpu())


@pytest.mark.parametrize("name,ratio", [("ref_int4_global", 0.5), ("channel_8", 0.0), ("channel_1_max", 0.0)])
@pytest.mark.parametrize("variant", list(FORMULA_MAXIMA))
def test_formulas_bf16(name, ratio, variant):
    case = formula_case(name, ratio, variant, 3, 37, 576, BF16)
    check_formula(case, *case.cpu())


def minus8_message(case):
    """A ref_int4_global message whose first lo row of every window is all code -8 (nibble 8).  No input encodes to
    it - the window max is taken over the very rows it scales, so x / m * 7 never passes -7 - but the format has the
    code and the decoder must give -8 / 7 * m.  Returns (message, row index per window)."""
    msg, L, _ = case.cpu()
    msg = msg.clone()
    rb = L.row_bytes(L.lo_fmt)
    for b in range(case.B):
        o = L.off_lo + b * L.k * rb
        msg[o:o + rb] = 0x88
    return msg, L, [b * case.S + int(np.nonzero(case.lo[b])[0][0]) for b in range(case.B)]


def check_minus8(case, y, rows):
    m = np.array(case.info["maxima"], dtype=np.float32)
    exp = (np.float32(-8) / np.float32(7) * m).astype(np.float64)
    for b, r in enumerate(rows):
        assert (y[r].double().numpy() == exp[b]).all(), (b, y[r, :4], exp[b])


@pytest.mark.parametrize("variant", list(FORMULA_MAXIMA))
def test_window_code_minus8_decodes(variant):
    case = formula_case("ref_int4_global", 0.5, variant, 3, 64, 128)
    msg, L, rows = minus8_message(case)
    check_minus8(case, C.decode(msg, case.spec, L, F32), rows)
    # and the most negative value an input can hold, -max, encodes to -7 (decode -m exactly)
    x = case.x.float().view(case.B, case.S, case.H)
    _, _, y = case.cpu()
    for b, m in enumerate(case.info["maxima"]):
        sel = torch.from_numpy(case.lo[b])[:, None] & (x[b] == -m)
        assert sel.any() and (y.view_as(x)[b][sel] == -m).all()


# ---- family 3: MX grids -------------------------------------------------------------------------------------------
MX_CODECS = ["mxfp4", "mxfp8", "mixed_mxfp4_mxfp8", "mxfp4_keep"]


def mx_params():
    return [(n, r, *shp) for n in MX_CODECS for r in ((0.5, 1.0) if C.get_codec(n).uses_ratio else (0.0,))
            for shp in MX_SHAPES]


@lru_cache(maxsize=None)
def mx_case(name, ratio, B, S, H, dtype=F32):
    """Every 32-channel block holds a pin that makes its scale X = 2^X_WINDOWS[window] - 6.0 (fp4) / 448 (fp8) times
    X, in every third block 7.9 X (fp4: saturates to 6) / 511.9 X (fp8: clamps to 448) - and walks through mx_list:
    every midpoint of the grid (E4M3's subnormal ones included), +-1 ulp, signed zeros, values that clamp."""
    spec = C.get_codec(name)
    lo = lo_mask(spec, ratio, importance(B, S))
    fmt, _ = row_formats(spec, lo, dtype)
    nb = H // 32
    T, D = np.zeros((B * S, H)), np.zeros((B * S, H), dtype=np.int64)
    for f in (W.FMT_MXFP4, W.FMT_MXFP8):
        rows = np.nonzero(np.where(np.isin(fmt, W.MX_FORMATS), fmt, W.FMT_MXFP4) == f)[0]   # native rows: fp4 lists
        if not len(rows):
            continue
        i = np.arange(len(rows) * nb)
        top, over = (6.0, 7.9) if f == W.FMT_MXFP4 else (448.0, 511.9 if dtype == F32 else 510.0)   # bf16(511.9) = 512
        pins = np.where(i % 3 == 0, over, top) * np.where(i % 2 == 0, 1.0, -1.0)
        Tu, Du = units(*mx_list(f), pins, 32)
        T[rows], D[rows] = Tu.reshape(len(rows), H), Du.reshape(len(rows), H)
    X = np.repeat(2.0 ** np.array(X_WINDOWS[:B], dtype=np.float64), S)[:, None]
    return new_case(name, ratio, B, S, H, realize(T * X, D, dtype), fmt=fmt, X=X)


def check_mx_rows(case, msg, L, y, rows=None):
    """Rows of an MX format decode to the enumerated-grid reference exactly (fp4: the sign survives on zero codes);
    native rows are exact; single-format messages store the reference's E8M0 bytes."""
    fmt = row_formats(case.spec, case.lo, case.x.dtype)[0]
    x, got = case.x64, y.double().numpy()
    rows = np.ones(len(fmt), dtype=bool) if rows is None else rows
    for f in (W.FMT_MXFP4, W.FMT_MXFP8):
        sel = (fmt == f) & rows
        if not sel.any():
            continue
        dec, sb = mx_reference(x[sel], f)
        bad = got[sel] != dec
        assert not bad.any(), (f, int(bad.sum()), x[sel][bad][:4], got[sel][bad][:4], dec[bad][:4])
        if f == W.FMT_MXFP4:
            assert np.array_equal(np.signbit(got[sel]), np.signbit(x[sel]))
        if L.k == 0:
            assert np.array_equal(inline_scales(msg, L)[sel], sb)
    nat = np.isin(fmt, (W.FMT_F32, W.FMT_BF16)) & rows
    assert np.array_equal(got[nat], x[nat])


def check_mx(case, msg, L, y):
    check_mx_rows(case, msg, L, y)
    fmt, x, got = case.info["fmt"], case.x64 / case.info["X"], y.double().numpy() / case.info["X"]
    # the named cases, spelled out: saturation at 6, the clamp at 448, signed zeros
    for f, over, top in ((W.FMT_MXFP4, 7.9, 6.0), (W.FMT_MXFP8, 511.9, 448.0)):
        sel = (fmt == f)[:, None] & (np.abs(x) > top)
        if (fmt == f).any():
            assert sel.any() and (np.abs(got[sel]) == top).all()
            assert case.x.dtype != F32 or (np.abs(x[sel]) == float(np.float32(over))).any()
    z = (fmt == W.FMT_MXFP4)[:, None] & (np.abs(x) < 0.25)
    assert not z.any() or ((got[z] == 0).all() and np.signbit(got[z]).any() and (~np.signbit(got[z])).any())


def test_mx_cases_cover_every_midpoint():
    for name, f in (("mxfp4", W.FMT_MXFP4), ("mxfp8", W.FMT_MXFP8)):
        case = mx_case(name, 0.0, 3, 37, 96)
        grid = MX_GRID[f][0]
        mid = (grid[:-1] + grid[1:]) / 2
        v = (case.x64 / case.info["X"]).reshape(3, -1)
        for b in range(3):
            for m in np.concatenate([mid, -mid]):
                near = v[b][np.abs(v[b] - m) <= abs(m) * 2.0 ** -22]
                assert (near == m).any() and (np.abs(near) < abs(m)).any() and (np.abs(near) > abs(m)).any(), (name, m)


@pytest.mark.parametrize("name,ratio,B,S,H", mx_params())
def test_mx_grids(name, ratio, B, S, H):
    case = mx_case(name, ratio, B, S, H)
    check_mx(case, *case.cpu())


@pytest.mark.parametrize("name,ratio", [("mxfp4", 0.0), ("mxfp8", 0.0), ("mixed_mxfp4_mxfp8", 0.5)])
def test_mx_grids_bf16(name, ratio):
    case = mx_case(name, ratio, 3, 37, 96, BF16)
    check_mx(case, *case.cpu())


# ---- family 4: zero units -----------------------------------------------------------------------------------------
ZERO_CODECS = sorted(set(C.CODECS) - {"passthrough"})
ZERO_SHAPES = [(3, 64, 64), (3, 64, 128), (3, 64, 576), (3, 64, 896), (3, 37, 128)]


def gaussian(B, S, H, seed):
    return torch.randn(B * S, H, generator=torch.Generator().manual_seed(seed)) * 3


@lru_cache(maxsize=None)
def zero_case(name, B, S, H, variant="units"):
    """A Gaussian tensor with an all-zero token row (window 0, token 5), an all-zero 64-channel group (token 9) and
    32-channel block (token 11) inside non-zero rows, every lo row of window 1 zero (ref_int4_global: a window max of
    0), channel 7 of window 0 and the last channel of window 2 zero; variant "all": nothing but zeros."""
    spec = spec_of(name, H)
    ratio = 0.5
    lo = lo_mask(spec, ratio, importance(B, S))
    x = gaussian(B, S, H, 40 + H).view(B, S, H)
    g0 = 64 * min(1, H // 64 - 1)
    x[0, 5] = 0
    x[0, 9, g0:g0 + 64] = 0
    x[0, 11, 32:64] = 0
    x[1][torch.from_numpy(lo[1])] = 0
    x[0, :, 7] = 0
    x[2, :, H - 1] = 0
    if variant == "all":
        x = torch.zeros_like(x)
    return new_case(name, ratio, B, S, H, x.reshape(B * S, H).contiguous(), g0=g0)


def check_zeros(case, msg, L, y):
    spec, B, S, H, g0 = case.spec, case.B, case.S, case.H, case.info["g0"]
    x = case.x.numpy()
    got = y.numpy()
    assert np.isfinite(got).all()
    if spec.name == "rgroup_rot":          # a rotated group is zero where the whole group is
        zero = np.repeat((x.reshape(B * S, H // 64, 64) == 0).all(-1), 64, axis=1)
    else:
        zero = x == 0
    assert zero.any() and (got[zero] == 0).all()
    sc = scale_section(msg, L, spec)
    fmt, _ = row_formats(spec, case.lo, F32)
    if spec.scale_mode == W.SC_TOKEN:
        assert sc[5] == 0 and (sc[(x == 0).all(1)] == 0).all()
        ints = np.isin(fmt, INT_FMTS) & (x != 0).any(1)
        assert (sc[ints] > 0).all()
    elif spec.scale_mode == W.SC_WINDOW:
        assert sc[1] == 0 and ((x == 0).all() or sc[0] > 0)
    elif spec.scale_mode == W.SC_CHANNEL and spec.ch_kind == W.CH_MAXABS:
        assert sc[7] == 0 and sc[2 * H + H - 1] == 0
        assert np.array_equal(sc.reshape(B, H), np.abs(x.reshape(B, S, H)).max(1))
    if L.k == 0 and (L.hi_fmt in W.GRP_FORMATS or L.hi_fmt in W.MX_FORMATS):
        ins = inline_scales(msg, L)
        U = 64 if L.hi_fmt in W.GRP_FORMATS else 32
        unit_zero = (x.reshape(B * S, H // U, U) == 0).all(-1)
        assert unit_zero[5].all() and unit_zero[9, g0 // U] and unit_zero[11, 32 // U] | (U == 64)
        assert (ins[unit_zero] == 0).all() and (ins[~unit_zero] != 0).all()


@pytest.mark.parametrize("B,S,H", ZERO_SHAPES)
@pytest.mark.parametrize("variant", ["units", "all"])
@pytest.mark.parametrize("name", ZERO_CODECS)
def test_zero_units(name, variant, B, S, H):
    case = zero_case(name, B, S, H, variant)
    check_zeros(case, *case.cpu())


# ---- family 5: Hadamard rows --------------------------------------------------------------------------------------
ROT_PLANS = ["w2", "w3", "w4", "w8", "all_widths"]
ROT_SHAPES = [(2, 64, 64), (2, 64, 128), (2, 64, 576), (2, 64, 896), (2, 37, 576)]
ROT_PATTERNS = ("one_hot", "constant", "alternating", "all_max", "massive", "gaussian")


def rot_plan(kind, H):
    return all_widths(H) if kind == "all_widths" else (int(kind[1:]),) * (H // 64)


@lru_cache(maxsize=None)
def rot_case(kind, B, S, H):
    """rgroup_rot; group g of row r holds pattern (r + g) % 6: a one-hot c e_j, a constant c, c with alternating
    signs (the transform's sparse images: H64 maps them to 8c at one channel), all +2^100, Gaussian with one channel
    2^20 times the rest, plain Gaussian."""
    n, G = B * S, H // 64
    x = torch.randn(n, G, 64, generator=torch.Generator().manual_seed(50 + H))
    pat = (np.arange(n)[:, None] + np.arange(G)[None, :]) % len(ROT_PATTERNS)
    c = (1.0 + torch.arange(n * G).view(n, G) % 29) * 3.7 * torch.where(torch.arange(n * G).view(n, G) % 2 == 0, 1, -1)
    j = (5 * torch.arange(n)[:, None] + 11 * torch.arange(G)[None, :]) % 64
    alt = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    P = torch.from_numpy(pat)
    x = torch.where((P == 0)[..., None], torch.nn.functional.one_hot(j, 64) * c[..., None], x)
    x = torch.where((P == 1)[..., None], c[..., None].expand(n, G, 64), x)
    x = torch.where((P == 2)[..., None], c[..., None] * alt, x)
    x = torch.where((P == 3)[..., None], torch.full_like(x, 2.0 ** 100), x)
    big = torch.nn.functional.one_hot(j, 64).bool() & (P == 4)[..., None]
    x = torch.where(big, x.abs().clamp_min(0.5) * 2.0 ** 20, x)
    return new_case("rgroup_rot", 0.0, B, S, H, x.reshape(n, H).float().contiguous(), plan=rot_plan(kind, H), pat=pat)


def rotated_bound(x64, dec64, s, qmax):
    """Bound on |H64 x' / 8 - H64 x / 8| per element of a group, x' the decode and s the stored scale (all fp64):

    * the encoder's six fp32 butterfly levels: each add rounds by 2^-24 relative to a partial sum that is at most
      ||x||_1, so its y differs from the fp64 transform by at most 7 * 2^-24 * ||x||_1 / 8 (7 for (1 + u)^6 - 1);
    * the quantizer: half a step, plus the two roundings of y * fl(1 / s) in code space: (0.5 + qmax 2^-22) s;
    * the decoder: x'_i = fl(int * (s / 8)), one rounding of 2^-24 relative each, through the transform at most
      2^-24 * ||x'||_1 / 8; the issue's decode term max|y| 2^-23 stays on top."""
    l1x, l1d = np.abs(x64).sum(-1, keepdims=True), np.abs(dec64).sum(-1, keepdims=True)
    ymax = np.abs(hadamard_groups(x64)).max(-1, keepdims=True)
    return (0.5 + qmax * 2.0 ** -22) * s + ymax * 2.0 ** -23 + 2.0 ** -24 * (7 * l1x + l1d) / 8


def check_rot_rows(case, msg, L, y, rows=None):
    """Every group of the rotated rows within rotated_bound of the fp64 transform; the stored scale is
    max|fp64 transform| / qmax up to the butterflies' rounding."""
    n, H = case.x.shape
    G = H // 64
    x = case.x64.reshape(n, G, 64)
    got = y.double().numpy().reshape(n, G, 64)
    s = inline_scales(msg, L).astype(np.float64)[..., None]
    qmax = np.array([qmax_of_bits(b) for b in L.plan], dtype=np.float64)[None, :, None]
    rows = np.ones(n, dtype=bool) if rows is None else rows
    yx, yg = hadamard_groups(x), hadamard_groups(got)
    bound = rotated_bound(x, got, s, qmax)
    ok = (np.abs(yg - yx) <= bound) | ~rows[:, None, None]
    assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[0], np.abs(yg - yx)[~ok][:3], bound[~ok][:3])
    am = np.abs(yx).max(-1, keepdims=True)
    l1 = np.abs(x).sum(-1, keepdims=True)
    tol = 7 * 2.0 ** -24 * l1 / 8 / qmax + am / qmax * 2.0 ** -23
    assert ((np.abs(s - am / qmax) <= tol) | ~rows[:, None, None]).all()


def check_rot(case, msg, L, y):
    n, H = case.x.shape
    G = H // 64
    x = case.x64.reshape(n, G, 64)
    got = y.double().numpy().reshape(n, G, 64)
    pat = case.info["pat"]
    assert np.isfinite(got).all()
    ulp = np.spacing(np.abs(case.x.numpy().reshape(n, G, 64))).astype(np.float64)
    sparse = np.isin(pat, (0, 1, 2, 3))[..., None]
    # one-hot / constant / alternating / all-max groups: exactly 0 where x is 0, within 2 ulp elsewhere
    assert (got[sparse & (x == 0)] == 0).all()
    err = np.abs(got - x)
    bad = sparse & (x != 0) & (err > 2 * ulp)
    assert not bad.any(), (np.argwhere(bad)[0], got[bad][:3], x[bad][:3])
    for p in range(len(ROT_PATTERNS)):
        assert (pat == p).any()
    check_rot_rows(case, msg, L, y)


@pytest.mark.parametrize("B,S,H", ROT_SHAPES)
@pytest.mark.parametrize("kind", ROT_PLANS)
def test_hadamard_rows(kind, B, S, H):
    case = rot_case(kind, B, S, H)
    check_rot(case, *case.cpu())


# ---- family 6: the rounding bound on ordinary data; family 7: the ends of the exponent range --------------------------
BOUND_CODECS = sorted(set(C.CODECS) - {"passthrough", "channel_1_mean"})
BOUND_SHAPES = [(3, 64, 576), (3, 37, 128)]
BOUND_SCALES = (2.0 ** -60, 1.0, 2.0 ** 100)


@lru_cache(maxsize=None)
def bound_case(name, B, S, H):
    """One Gaussian tensor, window b scaled by BOUND_SCALES[b] (exact)."""
    x = gaussian(B, S, H, 60 + H).view(B, S, H) * torch.tensor(BOUND_SCALES[:B]).float().view(B, 1, 1)
    return new_case(name, 0.5, B, S, H, x.reshape(B * S, H).contiguous())


def check_bound(case, msg, L, y, windows=None):
    """Per element |decode - x| <= (0.5 + qmax 2^-22) s + max|x| 2^-23 in fp64, s the stored scale of the element's
    unit and max|x| the unit's: half a step, the two roundings of x * fl(1 / s) (or of x / m * qmax) in code space,
    and the decode multiply.  The stored scale must be the fp32 quotient max|x| / qmax.  MX rows: the enumerated-grid
    reference, exactly.  Rotated rows: check_rot_rows.  Native rows: exact."""
    spec, B, S, H = case.spec, case.B, case.S, case.H
    windows = range(B) if windows is None else windows
    rows = np.isin(np.arange(B * S) // S, list(windows))
    fmt, qrow = row_formats(spec, case.lo, case.x.dtype)
    x, got = case.x64, y.double().numpy()
    x32 = case.x.float().numpy()
    sc = scale_section(msg, L, spec)
    assert np.isfinite(got[rows]).all()
    check_mx_rows(case, msg, L, y, rows)
    if spec.name == "rgroup_rot":
        return check_rot_rows(case, msg, L, y, rows)

    def within(sel, s, am, qmax):                # sel: bool [n] rows or [n, H] elements; s, am, qmax broadcast to [n, H]
        s, am, qmax = (np.broadcast_to(np.asarray(a, dtype=np.float64), x.shape) for a in (s, am, qmax))
        bound = (0.5 + qmax * 2.0 ** -22) * s + am * 2.0 ** -23
        ok = (np.abs(got - x) <= bound) | ~(sel if sel.ndim == 2 else sel[:, None])
        assert ok.all(), (spec.name, int((~ok).sum()), np.argwhere(~ok)[0], np.abs(got - x)[~ok][:3], bound[~ok][:3])

    ints = np.isin(fmt, INT_FMTS) & rows
    if spec.scale_mode == W.SC_TOKEN and ints.any():
        am32 = np.abs(x32).max(1)
        assert np.array_equal(sc[ints], am32[ints] / qrow[ints].astype(np.float32))
        within(ints, sc.astype(np.float64)[:, None], am32[:, None], qrow[:, None])
    elif spec.scale_mode == W.SC_WINDOW and ints.any():
        m = np.array([np.abs(x32.reshape(B, S, H)[b][case.lo[b]]).max() for b in range(B)])
        assert np.array_equal(sc, m)
        mrow = np.repeat(m.astype(np.float64), S)[:, None]
        within(ints, mrow / spec.qmax_lo, mrow, spec.qmax_lo)
    elif spec.scale_mode == W.SC_CHANNEL:
        ch = np.abs(x32.reshape(B, S, H)).max(1)
        assert np.array_equal(sc.reshape(B, H), ch)
        chrow = np.repeat(ch.astype(np.float64), S, axis=0)
        within(rows, chrow / spec.qmax_lo, chrow, spec.qmax_lo)
    grp = (fmt == W.FMT_GRP) & rows
    if grp.any():
        qg = np.repeat(np.array([qmax_of_bits(b) for b in L.plan], dtype=np.float32), 64)[None, :]
        am32 = np.repeat(np.abs(x32.reshape(B * S, H // 64, 64)).max(-1), 64, axis=1)
        s32 = am32 / qg                                        # the format's scale: the fp32 quotient
        if L.k == 0:
            assert np.array_equal(inline_scales(msg, L)[grp], s32[grp][:, ::64])
        within(grp, s32, am32, qg)
    nat = np.isin(fmt, (W.FMT_F32, W.FMT_BF16)) & rows
    assert np.array_equal(got[nat], x[nat])


@pytest.mark.parametrize("B,S,H", BOUND_SHAPES)
@pytest.mark.parametrize("name", BOUND_CODECS)
def test_rounding_bound(name, B, S, H):
    case = bound_case(name, B, S, H)
    check_bound(case, *case.cpu())


# normal regime: the largest max-abs and one whose int8 scale (2^-120 / 127) is a denormal.  Two formats overflow
# fp32 long before 3e38 BY DEFINITION and get 2^120 in its place: rgroup_rot's butterflies sum 64 values before the
# scaling by 1/8, and the reference's channel_8 / channel_4 decode is code * max / qmax - the product first (both
# overflows are loud: Inf, and from there NaN)
ENDS_NORMAL = (3e38, 2.0 ** -120)
ENDS_OVERFLOW_BY_FORMAT = ("rgroup_rot", "channel_8", "channel_4")
ENDS_TINY = (2.0 ** -126, 1e-39)         # below 2^-100: the oracle itself is not meaningful (see test_exponent_ends)
ENDS_SHAPES = [(2, 64, 128), (2, 37, 576)]


@lru_cache(maxsize=None)
def ends_case(name, variant, B, S, H):
    """Window b is u * M_b with u uniform in [-1, 1] and one element of every 32-channel block +-1 exactly (its
    position moves with the row, so every row, group, block, window and channel has max-abs exactly M_b)."""
    M = list(ENDS_NORMAL if variant == "normal" else ENDS_TINY)
    if name in ENDS_OVERFLOW_BY_FORMAT and variant == "normal":
        M[0] = 2.0 ** 120
    g = torch.Generator().manual_seed(70 + H)
    u = (torch.rand(B * S, H // 32, 32, generator=g, dtype=torch.float64) * 2 - 1)
    r = torch.arange(B * S)
    pin = torch.nn.functional.one_hot((r[:, None] + 3 * torch.arange(H // 32)[None, :]) % 32, 32).bool()
    u = torch.where(pin, torch.where(r % 2 == 0, 1.0, -1.0)[:, None, None].double(), u)
    Mw = torch.tensor(M[:B], dtype=torch.float64).repeat_interleave(S).view(B * S, 1, 1)
    Mw = Mw.float().double()                                   # the fp32 value of the pin (1e-39: a denormal)
    x = (u * Mw).float().reshape(B * S, H).contiguous()
    return new_case(name, 0.5, B, S, H, x, M=[float(v) for v in Mw.view(B, S)[:, 0]])


def check_ends(case, msg, L, y):
    """normal: window 0 (3e38) every format, window 1 (2^-120) the integer and head-group formats: check_bound.
    Below 2^-100 (MX at 2^-120; every format at 2^-126 and 1e-39): decode finite and |decode| <= 2 max|x| per unit
    (every unit's max-abs is the window's M).  rgroup_rot: |decode| <= 64 max|x| - its decode is H64 (q s) / 8 with
    |q s| <= max|y| <= 8 max|x|, so even exact arithmetic promises no more than 8 max|y| at 2 bits."""
    B, S, H = case.B, case.S, case.H
    fmt, _ = row_formats(case.spec, case.lo, F32)
    got = y.double().numpy().reshape(B, S, H)
    M = case.info["M"]
    x = case.x64.reshape(B, S, H)
    for b in range(B):
        assert np.abs(x[b]).max() == M[b] and (np.abs(x[b].reshape(S, H // 32, 32)).max(-1) == M[b]).all()
    strict = []
    for b in range(B):
        mx = np.isin(fmt.reshape(B, S)[b], W.MX_FORMATS).any()
        if M[b] > 2.0 ** -100 or (M[b] == 2.0 ** -120 and not mx):
            strict.append(b)
        else:
            lim = 64 if case.spec.name == "rgroup_rot" else 2
            assert np.isfinite(got[b]).all() and (np.abs(got[b]) <= lim * M[b]).all(), (case.spec.name, b)
    if strict:
        check_bound(case, msg, L, y, strict)
    return strict


@pytest.mark.parametrize("B,S,H", ENDS_SHAPES)
@pytest.mark.parametrize("variant", ["normal", "tiny"])
@pytest.mark.parametrize("name", BOUND_CODECS)
def test_exponent_ends(name, variant, B, S, H):
    """CPU oracle.  At 2^-126 and 1e-39 it is finite and bounded but not accurate (int8_token at 1e-39: 1 / s
    overflows, every non-zero value decodes to +-max|x|), which is why those windows ask no more on either side."""
    case = ends_case(name, variant, B, S, H)
    check_ends(case, *case.cpu())


# ---- family 8: NaN and Inf ----------------------------------------------------------------------------------------
NONFINITE_CODECS = sorted(C.CODECS)
NONFINITE_SHAPES = [(3, 64, 128), (3, 37, 576)]
PLACEMENTS = ("first_last", "last_first", "unit_max")


@lru_cache(maxsize=None)
def nonfinite_case(name, placement, B, S, H):
    """A Gaussian tensor with one NaN and one Inf in window 0:

    * first_last: NaN in a lo row at channel 0 (first lane of its group and block), +Inf in a hi row at channel
      H - 1 (the last lane);
    * last_first: NaN in a hi row at channel 63 (last lane of group 0), -Inf in a lo row at channel 32 (first lane
      of block 1);
    * unit_max: NaN replaces the largest |x| of a lo row, +Inf the largest of a hi row.

    (A codec without a lo class has every row in the hi class; the two rows differ all the same.)"""
    spec = spec_of(name, H)
    lo = lo_mask(spec, 0.5, importance(B, S))
    x = gaussian(B, S, H, 80 + H)
    r_lo = int(np.nonzero(lo[0])[0][1]) if lo[0].any() else 3
    r_hi = int(np.nonzero(~lo[0])[0][2])
    assert r_lo != r_hi and r_lo < S and r_hi < S
    nan, inf = float("nan"), float("inf")
    if placement == "first_last":
        pos = {(r_lo, 0): nan, (r_hi, H - 1): inf}
    elif placement == "last_first":
        pos = {(r_hi, 63): nan, (r_lo, 32): -inf}
    else:
        pos = {(r_lo, int(x[r_lo].abs().argmax())): nan, (r_hi, int(x[r_hi].abs().argmax())): inf}
    clean = x.clone()
    for (r, c), v in pos.items():
        x[r, c] = v
    return new_case(name, 0.5, B, S, H, x, pos=list(pos), clean=clean)


def check_nonfinite(case, msg, L, y, y_clean):
    """(a) every element that was NaN / Inf decodes non-finite; (b) the windows without one decode as they do from
    the clean tensor (``y_clean``: the decode of the same tensor without the two values)."""
    S = case.S
    for r, c in case.info["pos"]:
        assert r < S and not torch.isfinite(case.x[r, c])
        assert not torch.isfinite(y[r, c]), (case.spec.name, (r, c), float(case.x[r, c]), float(y[r, c]))
    assert torch.equal(y[S:], y_clean[S:]) and torch.isfinite(y[S:]).all()


@lru_cache(maxsize=None)
def clean_cpu(name, placement, B, S, H):
    case = nonfinite_case(name, placement, B, S, H)
    msg, L = C.encode(case.info["clean"], case.spec, B, S, case.ratio, case.imp)
    return msg, C.decode(msg, case.spec, L, F32)


@pytest.mark.parametrize("B,S,H", NONFINITE_SHAPES)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", NONFINITE_CODECS)
def test_nonfinite(name, placement, B, S, H):
    case = nonfinite_case(name, placement, B, S, H)
    msg, L, y = case.cpu()
    m_clean, y_clean = clean_cpu(name, placement, B, S, H)
    check_nonfinite(case, msg, L, y, y_clean)
    w0 = window_bytes(L, case.spec, 0)
    assert np.array_equal(msg.numpy()[~w0], m_clean.numpy()[~w0])
    if case.spec.lo_fmt in W.MX_FORMATS or case.spec.hi_fmt in W.MX_FORMATS:
        check_mx_nonfinite(case, msg, L, y, y_clean)


def check_mx_nonfinite(case, msg, L, y, y_clean):
    """An MX block holding a NaN / Inf is stored with E8M0 byte 255 (OCP: NaN) and decodes to NaN in all 32
    channels; every other block of window 0 decodes as from the clean tensor."""
    fmt, _ = row_formats(case.spec, case.lo, F32)
    hit = np.zeros(y.shape, dtype=bool)
    for r, c in case.info["pos"]:
        if fmt[r] in W.MX_FORMATS:
            blk = slice(32 * (c // 32), 32 * (c // 32) + 32)
            assert torch.isnan(y[r, blk]).all()
            hit[r, blk] = True
            if L.k == 0:
                assert inline_scales(msg, L)[r, c // 32] == 255
        else:
            hit[r, c] = True
    keep = torch.from_numpy(~hit)
    assert torch.equal(y[keep], y_clean[keep])
    if L.k == 0:
        assert (inline_scales(msg, L) == 255).sum() == sum(fmt[r] in W.MX_FORMATS for r, _ in case.info["pos"])

