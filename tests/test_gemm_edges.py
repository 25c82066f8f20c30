"""The GEMM family and the fused LM head + cross entropy on ragged shapes and hard rows, on the CPU paths of
``ops.linear``, ``ops.linear_h3``, ``ops.head_nll`` and ``ops.head_nll_h3``: the cases of ``helpers.gemm_case`` /
``helpers.nll_case`` at every M of ``GEMM_EDGE_M`` stay within the derived, component-wise caps against fp64 (so the
caps are satisfiable by the reference alone), the kinds meet their conditions, and the component-wise measure catches
seeded faults.  test_gemm_edges_gpu.py runs the same cases, through the same functions, on the HIP kernels; the CPU
results are its yardstick."""
import math
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

import helpers as T
from llm_inference_in_distributed_edge_networks_amd import ops
from llm_inference_in_distributed_edge_networks_amd.ops import reference as R

H3_EPIS = ["plain", "bias", "resid", "bias_resid", "rscale", "colscale", "inplace", "gelu", "swiglu"]
BF16_EPIS = ["none", "bias", "resid", "bias_resid", "gelu", "swiglu", "norm", "ssq"]
ACT_EPIS = ("gelu", "swiglu")
TILES = (128, 224, 256)
# 128 (one block, two wave columns) and 384; 256 and 1152 (N % 256 == 128 with tn >= 4: the half-used last column
# tile); 896 = 4 x 224
TILE_N = {128: (128, 384), 224: (896,), 256: (256, 1152)}
EDGE_K = (64, 128, 192)       # per plane: one paired K-tile pair / three K-tiles on the h3 kernels; bf16: 1, 2, 3 K-tiles
LONG_K, LONG_M = 896, (17, 257)
NORM_EPS = 1e-6
Check = namedtuple("Check", "name units cap")
Result = namedtuple("Result", "got ref checks")


def tile_fits(N, epi, tile):
    """The (N, epilogue) cells the forced tile really runs (gemm.hip ``launch`` / ``use_224``): 224-wide tiles take the
    plain / bias / residual epilogues of N % 224 == 0 shapes that 256 does not divide; 256-wide tiles N % 256 == 0, or
    N % 128 == 0 with at least four column tiles (not SwiGLU, whose gate / up pairs must not straddle a half-used
    tile).  Every other cell falls back to the 128x128 kernel and is left to tile 128."""
    if tile == 128:
        return True
    if tile == 224:
        return N % 224 == 0 and N % 256 != 0 and epi not in ACT_EPIS
    return N % 256 == 0 or (N % 128 == 0 and N >= 768 and epi != "swiglu")


def shapes(path, tile, epi):
    """(M, N, K) of one (path, tile, epilogue): every edge M at the short K, one long K at two M.  The bf16 256x224
    kernel needs two K-tiles (``use_224``: K = 64 runs the 128x128 kernel)."""
    out = []
    for N in TILE_N[tile]:
        if not tile_fits(N, epi, tile):
            continue
        ks = [K for K in EDGE_K if not (path == "bf16" and tile == 224 and K < 128)]
        out += [(M, N, K) for K in ks for M in T.GEMM_EDGE_M] + [(M, N, LONG_K) for M in LONG_M]
    return out


def kind_epis(path, kind):
    """Every epilogue on ``rand`` and ``zero_rows`` (rows that must come out as exactly bias / residual); the input
    kinds that stress the accumulation run the plain GEMM and the bias + residual one."""
    full = BF16_EPIS if path == "bf16" else H3_EPIS
    return full if kind in ("rand", "zero_rows") else [full[0], "bias_resid"]


@lru_cache(maxsize=8)
def aux_case(M, N):
    """bias [N], residual [M, N], row scale [M] in [0.5, 1.5), column scale [N] (fp32, seeded by the shape)."""
    g = torch.Generator().manual_seed(31 * M + N)
    return {"bias": 0.1 * torch.randn(N, generator=g), "resid": torch.randn(M, N, generator=g),
            "rs": torch.rand(M, generator=g) + 0.5, "cs": 1 + 0.3 * torch.randn(N, generator=g)}


@lru_cache(maxsize=4)
def h3_case(kind, M, N, K, two_term):
    x, w = T.gemm_case(kind, M, N, K, T.gemm_seed(M, N, K))
    if two_term:
        w = w.bfloat16().float()           # checkpoint values: exact in fp16 after the scale
    a3, w3, alpha, sx, sw = T.h3_operands(x, w, two_term)
    pe, Se, Kx = T.h3_exact(a3, w3, 1.0)   # (alpha and the row / column scales are applied per epilogue)
    pf, Sf = T.gemm_exact(x, w)
    floor = T.h3_lo_floor(x, w, sx, sw) if kind in ("rowmag", "outlier") else None
    return dict(x=x, w=w, a3=a3, w3=w3, alpha=alpha, sx=sx, sw=sw, pe=pe, Se=Se, Kx=Kx, pf=pf, Sf=Sf, floor=floor)


def h3_run(kind, M, N, K, two_term, epi, dev="cpu", case=None):
    """One h3 GEMM on ``dev`` and its two component-wise checks against fp64: ``arith`` from the planes (exact inputs:
    fp32 accumulation only, cap (Kx + 2) 2^-23 S) and ``fid`` from x and w (the cap gains 2^-21 S and, on rowmag and
    outlier, the lo planes' floor)."""
    c, aux = case or h3_case(kind, M, N, K, two_term), aux_case(M, N)
    bias = aux["bias"] if epi in ("bias", "bias_resid", "gelu") else None
    resid = aux["resid"] if epi in ("resid", "bias_resid", "colscale", "inplace") else None
    rs = aux["rs"] if epi in ("rscale", "colscale") else None
    cs = aux["cs"] if epi == "colscale" else None
    act = {"gelu": "gelu", "swiglu": "swiglu_il"}.get(epi)
    n_mul = 1 + (cs is not None)
    pe, Se = T.scale_ref(c["pe"], c["Se"], c["alpha"], rs, cs)
    pf, Sf = T.scale_ref(c["pf"], c["Sf"], 1.0, rs, cs)
    floor = 0.0 if c["floor"] is None else T.scale_ref(c["floor"], c["floor"], 1.0, rs, cs)[1]
    ref_e, Seff_e, e_e = T.epilogue_ref(pe, Se, bias, resid, act, n_mul)
    ref_f, Seff_f, e_f = T.epilogue_ref(pf, Sf, bias, resid, act, n_mul, floor)
    so = R.h3_scale(float(ref_f.abs().max()))

    def d(t):
        return None if t is None else t.to(dev)
    rd = d(resid)
    if resid is not None and dev == "cpu":
        rd = resid.clone()                      # (the in-place case writes into it)
    y = ops.linear_h3(d(c["a3"]), d(c["w3"]), c["alpha"], d(bias), rd, act, out=rd if epi == "inplace" else None,
                      rscale=d(rs), out_scale=so, colscale=d(cs))
    if epi == "inplace":
        assert y.data_ptr() == rd.data_ptr()
    y = y.cpu()
    if act is not None:
        assert y.dtype == torch.float16 and y.shape == (M, 2 * ref_f.shape[1])
        assert float(y.float().abs().max()) <= 2.0 ** 15, "planes above 2^15"
        y = R.h3_to_f32(y, so)
        e_e, e_f = e_e + T.plane_out_err(ref_e, so), e_f + T.plane_out_err(ref_f, so)
    cap = T.acc_cap_units(c["Kx"])
    return Result(y, ref_f, [Check("arith", T.gemm_units(y, ref_e, Seff_e, e_e), cap),
                             Check("fid", T.gemm_units(y, ref_f, Seff_f, e_f), cap + T.H3_DROPPED_UNITS)])


@lru_cache(maxsize=4)
def bf16_case(kind, M, N, K):
    x, w = (t.bfloat16() for t in T.gemm_case(kind, M, N, K, T.gemm_seed(M, N, K)))
    p, S = T.gemm_exact(x.float(), w.float())
    return dict(x=x, w=w, p=p, S=S)


def bf16_run(kind, M, N, K, epi, dev="cpu", case=None):
    """One bf16 GEMM on ``dev`` against fp64 on the bf16-rounded inputs: one bf16 ulp of the output, 2^-8 |ref|, plus
    the accumulation cap (K + 2) 2^-23 S.  ``norm``: the fused RMSNorm row scale (with bias and residual); ``ssq``:
    the plain GEMM with ``want_ssq``."""
    c, aux = case or bf16_case(kind, M, N, K), aux_case(M, N)
    bias = aux["bias"].bfloat16() if epi in ("bias", "bias_resid", "gelu", "norm") else None
    resid = aux["resid"].bfloat16() if epi in ("resid", "bias_resid", "norm") else None
    act = {"gelu": "gelu", "swiglu": "swiglu_il"}.get(epi)
    p, S, n_mul = c["p"], c["S"], 1
    xd, norm = c["x"].to(dev), None
    if epi == "norm":
        # the row scale from the device's own sum-of-squares partials and rsqrt: a few fp32 roundings of the product
        norm, n_mul = (ops.row_ssq(xd), NORM_EPS), 8
        rs64 = torch.rsqrt(c["x"].double().pow(2).sum(1) / K + NORM_EPS)
        p, S = T.scale_ref(p, S, 1.0, rs64)
    ref, Seff, e = T.epilogue_ref(p, S, None if bias is None else bias.float(), None if resid is None else
                                  resid.float(), act, n_mul)
    y = ops.linear(xd, c["w"].to(dev), None if bias is None else bias.to(dev),
                   None if resid is None else resid.to(dev), act, norm=norm, want_ssq=epi == "ssq")
    got = y.float().cpu()
    checks = [Check("out", T.gemm_units(got, ref, Seff, e + 2.0 ** -8 * ref.abs()), T.acc_cap_units(K))]
    if epi == "ssq":
        parts = y._edge_ssq.double().cpu()
        assert parts.shape[0] == M and N % parts.shape[1] == 0
        width = N // parts.shape[1]                       # 64-column slabs; 112 on the 256x224 kernel
        want = got.double().pow(2).view(M, -1, width).sum(-1)   # of the stored (rounded) values, no cancellation
        checks.append(Check("ssq", T.gemm_units(parts, want, want), T.acc_cap_units(width)))
    return Result(got, ref, checks)


def run(path, kind, M, N, K, epi, dev="cpu", case=None):
    """``case``: an uncached ``bf16_case`` / ``h3_case`` (large shapes that should not stay in the caches)."""
    if path == "bf16":
        return bf16_run(kind, M, N, K, epi, dev, case)
    return h3_run(kind, M, N, K, path == "h3_2", epi, dev, case)


@lru_cache(maxsize=None)
def oracle_units(path, kind, M, N, K, epi):
    """The CPU fp32 oracle's own error on the case, per check: the yardstick printed next to the kernels'."""
    return {c.name: c.units for c in run(path, kind, M, N, K, epi).checks}


def check_exact(path, kind, M, K, epi, res):
    """The kinds with an exact answer: ``onehot`` through the plain GEMM is bit-exact (the bf16 GEMM: the bf16
    rounding of the exact product); the all-zero rows of ``zero_rows`` come out as exactly the epilogue of a zero
    product - bias, residual or their one fp32 sum - and finite."""
    bf = path == "bf16"
    if kind == "onehot" and epi in ("plain", "none"):
        want = res.ref.float().bfloat16().float() if bf else res.ref.float()
        assert torch.equal(res.got, want), (path, kind, M, K, epi)
    if kind == "zero_rows" and epi not in ("swiglu", "gelu"):
        rows = sorted({0, M // 2, M - 1})
        want = res.ref[rows].float()                # (one fp32 add of fp32 / bf16 terms: fp64 rounds to the same)
        want = want.bfloat16().float() if bf else want
        assert torch.equal(res.got[rows], want), (path, kind, M, K, epi)
    if kind == "zero_rows" and epi == "swiglu":
        assert not res.got[sorted({0, M // 2, M - 1})].any()


def all_shapes(path, epi):
    return sorted({s for tile in TILES for s in shapes(path, tile, epi)})


# ---- 1. the CPU paths stay within the derived caps; the kinds' conditions ------------------------------------------
@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("path", ["bf16", "h3_2", "h3_3"])
def test_cpu_within_caps(path, kind):
    for epi in kind_epis(path, kind):
        for M, N, K in all_shapes(path, epi):
            if N == 1152 and K != 64 and M not in (1, 129, 257):
                continue                             # (the widest shape at a few M: the CPU paths have no tiles)
            res = run(path, kind, M, N, K, epi)
            for c in res.checks:
                assert c.units <= c.cap, (path, kind, epi, M, N, K, c)
            check_exact(path, kind, M, K, epi, res)


@pytest.mark.parametrize("M,N,K", [(17, 128, 64), (257, 896, 128)])
def test_kind_conditions(M, N, K):
    """cancel: |ref| <= 2^-8 sum |x||w| on every element, in fp32 and after bf16 rounding.  Every kind: planes finite
    and at most 2^15; the two-term weight really is a single plane.  onehot: the CPU h3 oracle's error is 0.0."""
    x, w = T.gemm_case("cancel", M, N, K, T.gemm_seed(M, N, K))
    for xx, ww in ((x, w), (x.bfloat16().float(), w.bfloat16().float())):
        p, S = T.gemm_exact(xx, ww)
        assert float((p.abs() <= 2.0 ** -8 * S).double().mean()) == 1.0
    for kind in T.GEMM_KINDS:
        for two_term in (True, False):
            c = h3_case(kind, M, N, K, two_term)
            for t in (c["a3"], c["w3"]):
                assert torch.isfinite(t.float()).all() and float(t.float().abs().max()) <= 2.0 ** 15
            assert c["w3"].shape[1] == (K if two_term else 3 * K)
    for path in ("h3_2", "h3_3"):
        res = run(path, "onehot", M, N, K, "plain")
        assert float((res.got.double() - res.ref).abs().max()) == 0.0


# ---- LM head + cross entropy -----------------------------------------------------------------------------------------
NLL_PATHS = ["bf16", "h3_2", "h3_3"]
NLL_SMALL = [(V, 64) for V in (128, 384)]                     # the 128x128 kernel
NLL_BIG = [(V, 64) for V in (65536, 65536 + 128)]             # ceil(R / 256) ceil(V / 256) >= 256: four-wave tiles


@lru_cache(maxsize=6)
def nll_inputs(path, kind, R_, V, K):
    """The case as the path sees it - bf16: both operands rounded; h3_2: bf16-valued weights; h3_3: fp32 - with its
    fp64 reference and cap."""
    h, w, t = T.nll_case(kind, R_, V, K, T.nll_seed(R_, V, K))
    if path == "bf16":
        h, w = h.bfloat16().float(), w.bfloat16().float()
        units = T.acc_cap_units(K)
    else:
        if path == "h3_2":
            w = w.bfloat16().float()
        units = T.acc_cap_units((2 if path == "h3_2" else 3) * K) + T.H3_DROPPED_UNITS
    ref = T.nll_ref(h, w, t)
    return h, w, t, ref, T.nll_cap(ref, units)


def nll_run(path, kind, R_, V, K, dev="cpu"):
    """-> (NLL [R] on ``dev``, max |err| / cap over the rows, max |err|)."""
    h, w, t, ref, cap = nll_inputs(path, kind, R_, V, K)
    if path == "bf16":
        got = ops.head_nll(h.bfloat16().to(dev), w.bfloat16().to(dev), t.to(dev))
    else:
        a3, w3, alpha, _, _ = T.h3_operands(h, w, path == "h3_2")
        got = ops.head_nll_h3(a3.to(dev), w3.to(dev), alpha, t.to(dev))
    return (got.cpu(),) + T.nll_err(got, ref, cap)


@lru_cache(maxsize=None)
def nll_oracle(path, kind, R_, V, K):
    return nll_run(path, kind, R_, V, K)[1:]


@pytest.mark.parametrize("kind", T.NLL_KINDS)
@pytest.mark.parametrize("path", NLL_PATHS)
def test_nll_cpu_within_caps(path, kind):
    for V, K in NLL_SMALL + NLL_BIG[1:]:
        for R_ in (T.NLL_EDGE_R if V < 1000 else (129,)):
            _, ratio, err = nll_run(path, kind, R_, V, K)
            assert ratio <= 1.0, (path, kind, R_, V, ratio, err)


def test_nll_kind_conditions():
    """The targets pin every offset of one slab, both ends of the vocabulary and both slabs of the partial tile; the
    kinds are what they say: flat = log V, peak60 ~ 0, far60 in 54..66 with maximum and target in different slabs,
    shift200 with every logit near -200, tie with the exact maximum three times."""
    V, K, R_ = 65536 + 128, 64, 129
    t = T.nll_targets(R_, V)
    assert sorted((t[8:72] % 64).tolist()) == list(range(64)) and len(set((t[8:72] // 64).tolist())) == 1
    assert {0, V - 1, 65536 - 64, 65536 - 1}.issubset(set(t.tolist()))
    assert {int(c) // 64 for c in t if c >= 65536} == {1024, 1025}
    ref = {kind: nll_inputs("h3_3", kind, R_, V, K) for kind in T.NLL_KINDS}
    assert float((ref["flat"][3][0] - math.log(V)).abs().max()) < 1e-12
    assert float(ref["peak60"][3][0].max()) < 1e-9
    far = ref["far60"]
    # (60 minus the target's own N(0, 1) logit; a few rows share a column with another row's structure)
    assert 54 <= float(far[3][0].quantile(0.05)) and float(far[3][0].quantile(0.9)) <= 66
    assert float(far[3][0].min()) > 40
    lg = far[0].double() @ far[1].double().t()
    assert bool((lg.argmax(-1) // 64 != far[2] // 64).all())
    sh = ref["shift200"]
    assert float((sh[0].double() @ sh[1].double().t()).max()) < -180
    tie = ref["tie"]
    lg = tie[0].float() @ tie[1].float().t()
    n_max = (lg == lg.amax(-1, keepdim=True)).sum(-1)
    assert float((n_max >= 2).float().mean()) > 0.9 and float((n_max >= 3).float().mean()) > 0.4


# ---- 2. seeded faults: what the component-wise measure catches, and what the global measures let through ------------
def old_h3(got, ref):
    """test_f32_gpu.py's measure and limit: max |err| / max |ref| < 2e-6."""
    return float((got.double() - ref).abs().max() / ref.abs().max()) < 2e-6


def old_bf16(got, ref):
    """test_kernels_gpu.py's: |err| <= 3e-2 + 2e-2 |ref| on every element."""
    return bool(((got.double() - ref).abs() <= 3e-2 + 2e-2 * ref.abs()).all())


def _swap_rows(y, M):
    r = M - 5                                  # inside the last partial row tile of every tile height
    y[[r, r ^ 8]] = y[[r ^ 8, r]]
    return y


def _shift_slab(y, M):
    y[:, 64:128] = torch.roll(y[:, 64:128], 4, dims=1)
    return y


GEMM_FAULTS = {"swap_rows": _swap_rows, "shift_slab": _shift_slab}


def _verdicts(name, kind, path, got, res_ref, units, cap):
    new_fails = units > cap
    old_passes = (old_bf16 if path == "bf16" else old_h3)(got, res_ref)
    print(f"GEMMFAULT {name} {path} {kind} units {units:.3g} cap {cap:.3g} new_fails {new_fails} "
          f"old_passes {old_passes}")
    return new_fails


@pytest.mark.parametrize("kind", ["rand", "outlier", "rowmag"])
def test_fault_lo_plane_tile(kind):
    """The lo plane of the first 64-wide K-tile zeroed for one 16-row group (rows 16..31), as an operand fault of the
    oracle.  Every kind catches it against the cap alone (1300 units against 516 at K = 128: 64 terms that each lose
    2^-12 of their product); ``outlier`` by the widest margin, its massive channel 3 sitting in that tile."""
    M, N, K = 129, 128, 128
    c = h3_case(kind, M, N, K, True)
    a3 = c["a3"].clone()
    a3[16:32, K:K + 64] = 0
    got = ops.linear_h3(a3, c["w3"], c["alpha"])
    pe, Se = T.scale_ref(c["pe"], c["Se"], c["alpha"])
    units = T.gemm_units(got, pe, Se, T.U24 * pe.abs())
    good = oracle_units("h3_2", kind, M, N, K, "plain")["arith"]
    assert units > 4 * max(good, 1.0), (kind, units, good)     # far outside the oracle's own error
    assert _verdicts("lo_tile", kind, "h3_2", got, c["pf"], units, T.acc_cap_units(c["Kx"]))


@pytest.mark.parametrize("path", ["bf16", "h3_2"])
@pytest.mark.parametrize("kind", ["rand", "rowmag"])
@pytest.mark.parametrize("fault", sorted(GEMM_FAULTS))
def test_fault_output_mapping(fault, kind, path):
    """Rows r and r ^ 8 swapped inside the last partial row tile; one 64-column slab shifted by 4 columns - applied
    to a copy of the oracle's output.  Both fail the component-wise check on ``rand`` and on ``rowmag``, where the
    swapped rows sit 2^-11 and 2^-19 below the largest row and the bf16 tests' atol no longer sees them."""
    M, N, K = 255, 128, 64
    epi = "none" if path == "bf16" else "plain"
    res = run(path, kind, M, N, K, epi)
    got = GEMM_FAULTS[fault](res.got.clone(), M)
    if path == "bf16":
        c = bf16_case(kind, M, N, K)
        units, cap = T.gemm_units(got, res.ref, c["S"], 2.0 ** -8 * res.ref.abs()), T.acc_cap_units(K)
    else:
        c = h3_case(kind, M, N, K, True)
        units, cap = T.gemm_units(got, res.ref, c["Sf"], T.U24 * res.ref.abs()), T.acc_cap_units(c["Kx"]) + 8
    assert _verdicts(fault, kind, path, got, res.ref, units, cap)


def old_nll_bf16(got, ref):
    return bool(((got.double() - ref).abs() <= 2e-2 + 1e-2 * ref.abs()).all())     # test_head_nll


def old_nll_h3(got, ref):
    return float((got.double() - ref).abs().max()) < 2e-5                          # test_head_nll_h3


@pytest.mark.parametrize("kind", ["rand", "peak12", "flat"])
@pytest.mark.parametrize("fault", ["target+1", "target^4", "drop_partial"])
def test_fault_nll(fault, kind):
    """The target logit taken one column on, or from another lane group (target ^ 4); one 64-column LSE partial
    dropped - on the oracle's logits.  ``rand`` and ``peak12`` catch the wrong target (``flat`` cannot: every logit is
    equal); ``rand`` and ``flat`` catch the dropped partial, which moves the NLL by about 64 / V = 1e-3 (``peak12``
    only just: the peak holds most of the mass)."""
    R_, V, K = 129, 65536 + 128, 64
    h, w, t, ref, cap = nll_inputs("h3_3", kind, R_, V, K)
    lg = h @ w.t()
    tt = {"target+1": (t + 1) % V, "target^4": t ^ 4}.get(fault, t)
    if fault == "drop_partial":
        lg = lg.clone()
        lg[:, 64 * 700:64 * 701] = float("-inf")
    got = torch.logsumexp(lg, -1) - (h @ w.t()).gather(1, tt.view(-1, 1)).squeeze(1)
    ratio, err = T.nll_err(got, ref, cap)
    print(f"GEMMFAULT {fault} nll {kind} err {err:.3g} err/cap {ratio:.3g} new_fails {ratio > 1} "
          f"old_bf16_passes {old_nll_bf16(got, ref[0])} old_h3_passes {old_nll_h3(got, ref[0])}")
    assert ratio > 1 or (kind, fault == "drop_partial") in (("flat", False), ("peak12", True))
