"""AttnLRP attention backward cases for ragged windows and hard softmax rows (tests/helpers.py ``edge_case`` x
``lrp_dO``), on the CPU: every case has a finite fp64 reference (``helpers.lrp_all64``) that agrees with
``ops.reference.lrp_attn_bwd``; the two CPU yardsticks - the fp32 oracle and an emulation of the bf16 sweeps' rounding
points - meet the caps the HIP kernels are held to in test_lrp_edges_gpu.py; and those caps tell the causal backward
from one whose mask or tail is off by one."""
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

import helpers as T
from llm_inference_in_distributed_edge_networks_amd import ops
from llm_inference_in_distributed_edge_networks_amd.ops import reference as R

NAMES = T.LRP_OUTPUTS


def yard_f32(q, k, v, dO, S):
    """The CPU fp32 oracle (what the CPU configuration runs), fed the CPU fp32 forward's own o and LSE."""
    o, lse = ops.attention(q, k, T.vt_of(v, S), S, need_lse=True)
    return dict(zip(NAMES, ops.lrp_attn_bwd(q, k, v, o, dO, lse)))


def yard_bf16(qb, kb, vb, dOb, S):
    """The bf16 sweeps' arithmetic on the CPU: bf16 q, k, v, dO and o, the fp32 LSE, products accumulated in fp32,
    and P and dS rounded to bf16 before the second products (``pack8`` in csrc/lrp.hip)."""
    q, k, v, dO = (t.float() for t in (qb, kb, vb, dOb))
    o, lse = ops.attention(q, k, T.vt_of(v, S), S, need_lse=True)
    B, Hq = q.shape[:2]
    G = Hq // k.shape[1]
    kk, vv = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    oh = o.bfloat16().float().view(B, S, Hq, 64).permute(0, 2, 1, 3)
    dOh = dO.view(B, S, Hq, 64).permute(0, 2, 1, 3)
    D = 0.5 * (oh * dOh).sum(-1)
    mask = torch.ones(S, S, dtype=torch.bool).triu(1)
    p = torch.exp(q @ kk.transpose(-1, -2) - lse[..., None]).masked_fill(mask, 0.0)
    dS = p * (0.5 * dOh @ vv.transpose(-1, -2) - D[..., None])
    pb, dSb = p.bfloat16().float(), dS.bfloat16().float()
    return {"D": D, "rel": D.sum(-1), "dq": 0.5 * dSb @ kk, "dk": 0.5 * dSb.transpose(-1, -2) @ q,
            "dv": 0.5 * pb.transpose(-1, -2) @ dOh}


@lru_cache(maxsize=32)
def lrp_ref(kid, layout, S, dkind):
    """The fp32 case: inputs, fp64 reference and row magnitudes, caps, and the CPU fp32 oracle's outputs and errors;
    shared by the tests, never modified."""
    q, k, v = T.edge_case(kid, *layout, S)
    dO = T.lrp_dO(dkind, *layout, S)
    ref, mag = T.lrp_all64(q, k, v, dO, S)
    yard = yard_f32(q, k, v, dO, S)
    return SimpleNamespace(q=q, k=k, v=v, dO=dO, ref=ref, mag=mag, caps=T.lrp_caps("f32", kid, q, k, S), yard=yard,
                           yerr={n: T.lrp_err(n, yard[n], ref[n], mag[n]) for n in NAMES})


@lru_cache(maxsize=32)
def lrp_ref_bf16(kid, layout, S, dkind):
    """The same case rounded to bf16: the fp64 reference on the rounded inputs (what the bf16 sweeps are held to) and
    the bf16 emulation's outputs and errors."""
    c = lrp_ref(kid, layout, S, dkind)
    q, k, v, dO = (t.bfloat16() for t in (c.q, c.k, c.v, c.dO))
    ref, mag = T.lrp_all64(q.float(), k.float(), v.float(), dO.float(), S)
    yard = yard_bf16(q, k, v, dO, S)
    return SimpleNamespace(q=q, k=k, v=v, dO=dO, ref=ref, mag=mag, caps=T.lrp_caps("bf16", kid, q, k, S), yard=yard,
                           yerr={n: T.lrp_err(n, yard[n], ref[n], mag[n]) for n in NAMES})


@pytest.mark.parametrize("S", T.LRP_EDGE_S)
@pytest.mark.parametrize("kid", T.EDGE_KIND_IDS)
def test_cases(kid, S):
    for layout in T.LRP_LAYOUTS:
        B, Hq, Hkv = layout
        for dkind in T.LRP_DO_KINDS:
            c = lrp_ref(kid, layout, S, dkind)
            where = (kid, layout, S, dkind)
            assert all(torch.isfinite(r).all() for r in c.ref.values()), where
            assert all(torch.isfinite(m).all() and (m >= 0).all() for m in c.mag.values()), where
            assert torch.allclose(c.ref["rel"], c.ref["D"].sum(-1), rtol=0, atol=1e-12), where
            # the explicit form with the causal mask is ops.reference.lrp_attn_bwd in fp64
            q, k, v, dO = (t.double() for t in (c.q, c.k, c.v, c.dO))
            want = R.lrp_attn_bwd(q, k, v, c.ref["o"], dO, c.ref["lse"])
            for n, w in zip(NAMES, want):
                assert T.lrp_err(n, w, c.ref[n], c.mag[n]) < 1e-12, (n, where)
            if kid == "flat":           # q = 0: P_ij = 1 / (i + 1), so dv_j = 1/2 sum_{i >= j} dO_i / (i + 1)
                n_ = torch.arange(1, S + 1, dtype=torch.float64).view(1, 1, S, 1)
                dOh = dO.view(B, S, Hq, 64).permute(0, 2, 1, 3)
                dv = 0.5 * (dOh / n_).flip(2).cumsum(2).flip(2)
                assert torch.allclose(c.ref["dv"], dv, rtol=0, atol=1e-13), where
                assert not c.ref["dk"].any() and not c.mag["dk"].any(), where
            if dkind == "zero_head":    # the zeroed heads have magnitude 0 in every output (exact zeros are required)
                for n in NAMES:
                    assert not c.mag[n][0, :Hq // Hkv].any() and (Hq == 1 or not c.mag[n][:, 1].any()), (n, where)
            # the yardsticks meet the caps the kernels are held to
            for tag, cc in (("f32", c), ("bf16", lrp_ref_bf16(kid, layout, S, dkind))):
                for n in NAMES:
                    assert cc.yerr[n] <= cc.caps[n], (tag, n, where, cc.yerr[n], cc.caps[n])


# every wrong mask moves D, dq, dk and dv (``pad_last`` through the last row alone: D and dq in row S - 1, dv in key
# S - 1, dk in every key that row sees); rel is a sum that one key barely moves and is exempt
MUTANTS = {"mask+1": dict(shift=1), "mask-1": dict(shift=-1), "pad_last": dict(pad_last=True)}
MOVED = ("D", "dq", "dk", "dv")
# The bf16 caps are a few hundred times the fp32 ones.  dk and dv see every mutant at every length (a dropped key
# zeroes its dv row: error 1).  D and dq see ``pad_last`` only through the last row's own key, 1 / S of that row
# under ``flat`` and whatever the seed gives it under ``rand``: they must detect every mutant on every layout at
# these lengths (asserted: the list is the condition, not a report; the smallest mutant error / cap on the list is
# 1.8, off the list it falls to 0.16).
_S2 = [s for s in T.LRP_EDGE_S if s >= 2]
BF16_DETECTS = {("flat", "D"): _S2, ("flat", "dq"): [s for s in _S2 if s <= 129],
                ("rand", "D"): [2, 15, 17, 32, 64], ("rand", "dq"): [2, 15, 17, 32, 64, 257]}


def mutant_errors(c, S):
    """{(mutant, output): error of the yardstick's output against the mutant reference, on the case's own row
    magnitudes}."""
    out = {}
    for mut, kw in MUTANTS.items():
        bad, _ = T.lrp_all64(c.q.float(), c.k.float(), c.v.float(), c.dO.float(), S, **kw)
        for n in MOVED:
            out[mut, n] = T.lrp_err(n, c.yard[n], bad[n], c.mag[n])
    return out


@pytest.mark.parametrize("S", [s for s in T.LRP_EDGE_S if s >= 2])
@pytest.mark.parametrize("kid", ["rand", "flat"])
def test_detection(kid, S):
    """A condition on the cases: the yardsticks' outputs FAIL the caps against a reference whose causal mask is off by
    one in either direction, or that treats key S - 1 as padding, on every output the mutation moves (dk under
    ``flat`` is identically 0)."""
    for layout in T.LRP_LAYOUTS:
        c, cb = lrp_ref(kid, layout, S, "rand"), lrp_ref_bf16(kid, layout, S, "rand")
        for (mut, n), err in mutant_errors(c, S).items():
            if not (kid == "flat" and n == "dk"):
                assert err > c.caps[n], ("f32", mut, n, layout, err, c.caps[n])
        for (mut, n), err in mutant_errors(cb, S).items():
            if (kid == "flat" and n == "dk") or (n in ("D", "dq") and S not in BF16_DETECTS[kid, n]):
                continue
            assert err > cb.caps[n], ("bf16", mut, n, layout, err, cb.caps[n])
