"""The cases of test_lrp_edges.py on the HIP kernels: the AttnLRP attention backward sweeps in bf16 (csrc/lrp.hip
lrp_attn_delta / dkdv / dq) and fp32 (csrc/lrp_f32.hip lrp_attn_delta_f32 / dkdv_h3<GS> / dq_h3) at every length of
``LRP_EDGE_S`` (one off the 16-key wave slice, the 32-row staged tile and the 64-row block; S = 1 and 2), on five head
layouts (G = 1, 2, 7, 16), ten row kinds and three upstream gradients (Gaussian, the seed's last-row gradient, zeroed
heads), per row against fp64 on the cancellation-free scale (``helpers.lrp_err``); the inverse-RoPE pack kernels at
row counts that leave a partial last workgroup, on every dispatch branch; and both relevance engines on ragged
windows."""
import math

import pytest
import torch

import helpers as T
import test_lrp_edges as E
from llm_inference_in_distributed_edge_networks_amd import ops
from llm_inference_in_distributed_edge_networks_amd.models import TINY_NEOX, TINY_QWEN2, DecoderLM
from llm_inference_in_distributed_edge_networks_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = T.LRP_OUTPUTS

# Asserted bounds per kernel path, output and kind: twice the largest error measured on the MI355X over every length,
# layout and dO kind of that kind, rounded up to one digit (docs/RESULTS.md section 10; the kernels are
# deterministic), and never above the derived cap ``helpers.lrp_caps``.  Where twice the measured error is below
# 3e-7 > 2^-22, two fp32 roundings of the row's magnitude, the bound is 3e-7 (flat: exact scores; sink150: key 0 has
# probability 1.0) or the cap if that is lower; dk under ``flat`` is exactly 0.  The largest error / cap is 0.42
# (bf16 D), 0.39 and 0.37 (h3 dq and dv, on flat, whose caps are 4.4e-7 and 3.1e-6 with no score term).  h3 dv on
# sink150 is 100 x the CPU oracle (scores of 150 nats: an ulp of 1.5e-5 in the exponent, where the oracle's s - lse
# is exactly 0) and a tenth of its cap.
#   h3: the fp32 sweeps fed the GPU fp32 forward's o and LSE (the engine's path); dk_sum / dv_sum from gqa_sum=True
#   iso: the fp32 sweeps fed the fp64 o and LSE rounded to fp32 (the backward's own error)
#   bf16: the bf16 sweeps fed the GPU bf16 forward's o and LSE, against fp64 on the rounded inputs
MEASURED_BOUND = {
    "h3.D": {"rand": 4e-06, "flat": 3e-07, "sink30": 5e-06, "sink150": 3e-07, "diag60": 5e-06, "ramp7.5": 5e-06,
             "ramp8": 5e-06, "ramp8.5": 5e-06, "ramp16": 2e-05, "down40": 4e-06},
    "h3.rel": {"rand": 2e-06, "flat": 3e-07, "sink30": 3e-06, "sink150": 3e-07, "diag60": 3e-06, "ramp7.5": 4e-06,
               "ramp8": 5e-06, "ramp8.5": 4e-06, "ramp16": 6e-06, "down40": 2e-06},
    "h3.dq": {"rand": 2e-06, "flat": 4e-07, "sink30": 4e-06, "sink150": 3e-07, "diag60": 2e-06, "ramp7.5": 2e-06,
              "ramp8": 2e-06, "ramp8.5": 2e-06, "ramp16": 2e-06, "down40": 2e-06},
    "h3.dk": {"rand": 6e-06, "flat": 0.0, "sink30": 7e-06, "sink150": 3e-07, "diag60": 5e-06, "ramp7.5": 6e-06,
              "ramp8": 7e-06, "ramp8.5": 7e-06, "ramp16": 2e-05, "down40": 4e-06},
    "h3.dv": {"rand": 2e-05, "flat": 3e-06, "sink30": 4e-05, "sink150": 7e-05, "diag60": 3e-05, "ramp7.5": 4e-05,
              "ramp8": 4e-05, "ramp8.5": 4e-05, "ramp16": 5e-05, "down40": 2e-05},
    "h3.dk_sum": {"rand": 6e-06, "flat": 0.0, "sink30": 7e-06, "sink150": 3e-07, "diag60": 4e-06, "ramp7.5": 6e-06,
                  "ramp8": 6e-06, "ramp8.5": 7e-06, "ramp16": 1e-05, "down40": 4e-06},
    "h3.dv_sum": {"rand": 2e-05, "flat": 3e-06, "sink30": 4e-05, "sink150": 5e-05, "diag60": 3e-05, "ramp7.5": 4e-05,
                  "ramp8": 3e-05, "ramp8.5": 3e-05, "ramp16": 5e-05, "down40": 2e-05},
    "iso.D": {"rand": 3e-07, "flat": 3e-07},
    "iso.rel": {"rand": 3e-07, "flat": 3e-07},
    "iso.dq": {"rand": 3e-06, "flat": 3e-07},
    "iso.dk": {"rand": 4e-06, "flat": 0.0},
    "iso.dv": {"rand": 2e-05, "flat": 9e-07},
    "iso.dk_sum": {"rand": 4e-06, "flat": 0.0},
    "iso.dv_sum": {"rand": 2e-05, "flat": 9e-07},
    "bf16.D": {"rand": 5e-03, "flat": 3e-03, "sink30": 4e-03, "sink150": 3e-07, "diag60": 5e-03, "ramp7.5": 4e-03,
               "ramp8": 4e-03, "ramp8.5": 5e-03, "ramp16": 4e-03, "down40": 4e-03},
    "bf16.rel": {"rand": 3e-03, "flat": 3e-03, "sink30": 2e-03, "sink150": 3e-07, "diag60": 3e-03, "ramp7.5": 3e-03,
                 "ramp8": 4e-03, "ramp8.5": 3e-03, "ramp16": 3e-03, "down40": 3e-03},
    "bf16.dq": {"rand": 3e-03, "flat": 2e-03, "sink30": 3e-03, "sink150": 3e-07, "diag60": 3e-03, "ramp7.5": 2e-03,
                "ramp8": 2e-03, "ramp8.5": 3e-03, "ramp16": 2e-03, "down40": 2e-03},
    "bf16.dk": {"rand": 4e-03, "flat": 0.0, "sink30": 4e-03, "sink150": 3e-07, "diag60": 4e-03, "ramp7.5": 4e-03,
                "ramp8": 4e-03, "ramp8.5": 4e-03, "ramp16": 4e-03, "down40": 4e-03},
    "bf16.dv": {"rand": 8e-03, "flat": 8e-03, "sink30": 8e-03, "sink150": 3e-07, "diag60": 8e-03, "ramp7.5": 8e-03,
                "ramp8": 8e-03, "ramp8.5": 8e-03, "ramp16": 8e-03, "down40": 8e-03},
}


def bound(path, name, kid, caps):
    return min(caps[name.replace("_sum", "")], MEASURED_BOUND.get(f"{path}.{name}", {}).get(kid, math.inf))


def check(path, name, kid, layout, S, dkind, got, c):
    """Print the measured error (and its ratio to the CPU yardstick's own error on the case), then assert."""
    base = name.replace("_sum", "")
    err = T.lrp_err(name, got, c.ref[name], c.mag[name])
    y = c.yerr[base]
    print(f"LRPEDGE {path}.{name} {kid} {layout} S={S} dO={dkind} err {err:.3e} cap {c.caps[base]:.3e} yard {y:.3e} "
          f"ratio {err / max(y, 1e-30):.2f}")
    b = bound(path, name, kid, c.caps)
    assert err <= b, (path, name, kid, layout, S, dkind, err, b)


def scales(q, k, v):
    """in_scales of the fp16-plane kernels from the case's own maxima: powers of two with s |x| <= 2^15."""
    return tuple(R.h3_scale(float(t.abs().max())) for t in (q, k, v))


def f32_inputs(c, S):
    """The case on the GPU, its plane scales, and the GPU fp32 forward's o and LSE on the same planes."""
    sc = scales(c.q, c.k, c.v)
    q, k, v, dO = (t.to(DEV) for t in (c.q, c.k, c.v, c.dO))
    o, lse = ops.attention(q, k, T.vt_of(c.v, S).to(DEV), S, need_lse=True, in_scales=sc)
    return q, k, v, dO, o, lse, sc


def zero_heads_exact(out, layout, where):
    """``zero_head``: q head 1 of every window and kv group 0 of window 0 are exactly 0 in every output."""
    B, Hq, Hkv = layout
    G = Hq // Hkv
    for n, t in out.items():
        if n.endswith("_sum"):
            assert not t[0, 0].any(), (n, where)
            continue
        assert not t[0, :G].any(), (n, where)
        assert Hq == 1 or not t[:, 1].any(), (n, where)


@pytest.mark.parametrize("S", T.LRP_EDGE_S)
@pytest.mark.parametrize("kid", T.EDGE_KIND_IDS)
def test_f32_engine_path(kid, S):
    """The fp32 sweeps as the engine runs them: o and LSE from the GPU fp32 forward, per-q-head partials and group
    sums; every output within its bound, D / rel / dq identical between the two forms, two runs bit-identical."""
    for layout in T.LRP_LAYOUTS:
        for dkind in T.LRP_DO_KINDS:
            c = E.lrp_ref(kid, layout, S, dkind)
            q, k, v, dO, o, lse, sc = f32_inputs(c, S)
            got = dict(zip(NAMES, ops.lrp_attn_bwd(q, k, v, o, dO, lse, in_scales=sc)))
            gs = dict(zip(NAMES, ops.lrp_attn_bwd(q, k, v, o, dO, lse, gqa_sum=True, in_scales=sc)))
            again = dict(zip(NAMES, ops.lrp_attn_bwd(q, k, v, o, dO, lse, in_scales=sc)))
            torch.cuda.synchronize()
            where = (kid, layout, S, dkind)
            for n in NAMES:
                assert torch.equal(got[n], again[n]), ("not deterministic", n, where)
                check("h3", n, kid, layout, S, dkind, got[n], c)
            for n in ("D", "rel", "dq"):
                assert torch.equal(got[n], gs[n]), ("gqa_sum changes", n, where)
            for n in ("dk", "dv"):
                check("h3", n + "_sum", kid, layout, S, dkind, gs[n], c)
            if kid == "flat":
                assert not got["dk"].any() and not gs["dk"].any(), where
            if dkind == "zero_head":
                zero_heads_exact({**got, "dk_sum": gs["dk"], "dv_sum": gs["dv"]}, layout, where)


@pytest.mark.parametrize("S", T.LRP_EDGE_S)
@pytest.mark.parametrize("kid", ["rand", "flat"])
def test_f32_isolated(kid, S):
    """The fp32 sweeps fed the fp64 o and LSE rounded to fp32: only the backward's own error, same caps."""
    for layout in T.LRP_LAYOUTS:
        for dkind in T.LRP_DO_KINDS:
            c = E.lrp_ref(kid, layout, S, dkind)
            sc = scales(c.q, c.k, c.v)
            q, k, v, dO = (t.to(DEV) for t in (c.q, c.k, c.v, c.dO))
            o, lse = c.ref["o"].float().to(DEV), c.ref["lse"].float().contiguous().to(DEV)
            got = dict(zip(NAMES, ops.lrp_attn_bwd(q, k, v, o, dO, lse, in_scales=sc)))
            gs = dict(zip(NAMES, ops.lrp_attn_bwd(q, k, v, o, dO, lse, gqa_sum=True, in_scales=sc)))
            for n in NAMES:
                check("iso", n, kid, layout, S, dkind, got[n], c)
            for n in ("dk", "dv"):
                check("iso", n + "_sum", kid, layout, S, dkind, gs[n], c)


@pytest.mark.parametrize("S", T.LRP_EDGE_S)
@pytest.mark.parametrize("kid", T.EDGE_KIND_IDS)
def test_bf16(kid, S):
    """The bf16 sweeps on the rounded inputs, o and LSE from the GPU bf16 forward, against fp64 on the rounded
    inputs."""
    for layout in T.LRP_LAYOUTS:
        for dkind in T.LRP_DO_KINDS:
            c = E.lrp_ref_bf16(kid, layout, S, dkind)
            q, k, v, dO = (t.to(DEV) for t in (c.q, c.k, c.v, c.dO))
            o, lse = ops.attention(q, k, T.vt_of(c.v, S).to(DEV), S, need_lse=True)
            got = dict(zip(NAMES, ops.lrp_attn_bwd(q, k, v, o, dO, lse)))
            again = dict(zip(NAMES, ops.lrp_attn_bwd(q, k, v, o, dO, lse)))
            torch.cuda.synchronize()
            where = (kid, layout, S, dkind)
            assert max(c.caps.values()) <= 2e-2
            for n in NAMES:
                assert torch.equal(got[n], again[n]), ("not deterministic", n, where)
                check("bf16", n, kid, layout, S, dkind, got[n], c)
            if kid == "flat":
                assert not got["dk"].any(), where
            if dkind == "zero_head":
                zero_heads_exact(got, layout, where)


@pytest.mark.parametrize("layout", [(3, 4, 2), (2, 14, 2)])
@pytest.mark.parametrize("S", [1, 33, 65, 129])
def test_f32_window_equals_single(S, layout):
    """Every workgroup and the dO scale are per window: window b of a batch equals the B = 1 run of that window bit for
    bit, for a Gaussian dO and with zeroed heads (window 0's group 0 takes the ``mx == 0`` scale, the others do
    not), per-q-head partials and group sums."""
    B, Hq, Hkv = layout
    for dkind in ("rand", "zero_head"):
        c = E.lrp_ref("rand", layout, S, dkind)
        q, k, v, dO, o, lse, sc = f32_inputs(c, S)
        for gs in (False, True):
            full = ops.lrp_attn_bwd(q, k, v, o, dO, lse, gqa_sum=gs, in_scales=sc)
            for b in range(B):
                rows = slice(b * S, (b + 1) * S)
                one = ops.lrp_attn_bwd(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(),
                                       o[rows].contiguous(), dO[rows].contiguous(), lse[b:b + 1].contiguous(),
                                       gqa_sum=gs, in_scales=sc)
                for n, f_, o_ in zip(NAMES, full, one):
                    assert torch.equal(f_[b:b + 1], o_), (n, dkind, gs, b)


@pytest.mark.parametrize("S", [1, 33, 65])
def test_f32_dO_scale_equivariance(S):
    """dO's plane scale is a power of two from its per-head maxima: every output is bit-identical after unscaling
    under dO x 2^-40 and 2^+40 (test_lrp_attn_bwd_dynamic_range's check, at the ragged lengths)."""
    for layout in ((3, 4, 2), (2, 14, 2)):
        for dkind in T.LRP_DO_KINDS:
            c = E.lrp_ref("rand", layout, S, dkind)
            q, k, v, dO, o, lse, sc = f32_inputs(c, S)
            for gs in (False, True):
                base = ops.lrp_attn_bwd(q, k, v, o, dO, lse, gqa_sum=gs, in_scales=sc)
                for e in (-40, 40):
                    got = ops.lrp_attn_bwd(q, k, v, o, dO * 2.0 ** e, lse, gqa_sum=gs, in_scales=sc)
                    for n, g_, b_ in zip(NAMES, got, base):
                        assert torch.equal(g_ * 2.0 ** -e, b_), (n, layout, dkind, gs, e)


# ---- inverse RoPE + GQA sum + pack at row counts that leave a partial last workgroup --------------------------
def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    assert torch.isfinite(a).all()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


# (Hq, Hkv, rot_dim) per dispatch branch of rope_pack_h3 (W = (Hq + 2 Hkv) 64)
ROPE_BRANCHES = {"v4<5>": [(4, 2, 64), (4, 2, 16)],                # rot_dim % 8 == 0, W = 512 <= 1280
                 "v4<8>": [(8, 8, 64), (16, 4, 16)],               # W = 1536
                 "generic<32>": [(4, 2, 12), (16, 4, 12)],         # rot_dim % 8 != 0, W <= 2048
                 "generic<0>": [(32, 4, 64), (32, 4, 12)]}         # W = 2560 > 2048
# B * S = 1, 2, 3 (mod 4) rows with 4 rows per workgroup, S = 1 among them
ROPE_ROWS = [(1, 1), (2, 1), (3, 1), (3, 7), (2, 35), (1, 23)]


@pytest.mark.parametrize("B,S", ROPE_ROWS)
@pytest.mark.parametrize("branch", list(ROPE_BRANCHES))
def test_rope_pack_h3_partial_workgroups(branch, B, S):
    for Hq, Hkv, rot in ROPE_BRANCHES[branch]:
        W = (Hq + 2 * Hkv) * 64
        assert {"v4<5>": rot % 8 == 0 and W <= 1280, "v4<8>": rot % 8 == 0 and 1280 < W <= 2048,
                "generic<32>": rot % 8 != 0 and W <= 2048, "generic<0>": W > 2048}[branch]
        cos, sin = R.rope_tables(128, rot, 1e4)
        dq, dk, dv = (rnd(B, Hq, S, 64, seed=sd + S) for sd in (5, 6, 7))
        want = R.lrp_rope_pack(dq.double(), dk.double(), dv.double(), cos.double(), sin.double(), B, S, Hq, Hkv, rot,
                               0.125)
        dks, dvs = (t.view(B, Hkv, Hq // Hkv, S, 64).sum(2).contiguous() for t in (dk, dv))
        for form, (a, b) in (("partials", (dk, dv)), ("sums", (dks, dvs))):
            g3, gi = ops.lrp_rope_pack_h3(dq.to(DEV), a.to(DEV), b.to(DEV), cos.to(DEV), sin.to(DEV), B, S, Hq, Hkv,
                                          rot, 0.125)
            torch.cuda.synchronize()
            assert g3.shape == (B * S, 2 * W) and gi.shape == (B * S,), (form, Hq, Hkv, rot)
            assert float(g3.float().abs().max()) < 2 ** 15, (form, Hq, Hkv, rot)
            e = rel_err(R.h3_to_f32(g3.cpu()) * gi.cpu().view(-1, 1), want)
            assert e < 1e-6, (form, Hq, Hkv, rot, e)


@pytest.mark.parametrize("B,S", ROPE_ROWS)
def test_rope_pack_bf16_partial_workgroups(B, S):
    for Hq, Hkv, rot in ((4, 2, 64), (4, 2, 16), (14, 2, 64)):
        cos, sin = R.rope_tables(128, rot, 1e4)
        dq, dk, dv = (rnd(B, Hq, S, 64, seed=sd + S) for sd in (5, 6, 7))
        want = R.lrp_rope_pack(dq, dk, dv, cos, sin, B, S, Hq, Hkv, rot, 0.125)
        got = ops.lrp_rope_pack(dq.to(DEV), dk.to(DEV), dv.to(DEV), cos.to(DEV), sin.to(DEV), B, S, Hq, Hkv, rot,
                                0.125)
        assert got.shape == want.shape and rel_err(got, want) < 5e-3, (Hq, Hkv, rot)


# ---- both engines on ragged windows ------------------------------------------------------------------------------
RAGGED = [(3, 77), (2, 129), (1, 33)]
# The seed is the largest logit of each window's last row, and the relevance pass starts from that token's head row:
# where the two largest logits are closer than bf16 resolves, the bf16 engine may pick the other token and every
# table changes (on the first ids of tiny-qwen2 at (3, 77) they are 0.1 % and 0.3 % apart in two windows, and the
# bf16 tables differ from the fp32 ones by 90 %).  That is a property of the ids, not of a kernel: these (model, S)
# take the first seed of the sequence 2 + S + 1000 t on which every window's gap exceeds 2 % of the largest logit,
# twice the 1e-2 the bf16 seed logit is held to (asserted in test_engine_bf16_ragged).
RAGGED_SEED_STEP = {("tiny-qwen2", 77): 2}


def ragged_ids(cfg, B, S):
    seed = 2 + S + 1000 * RAGGED_SEED_STEP.get((cfg.name, S), 0)
    return torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("B,S", RAGGED)
@pytest.mark.parametrize("cfg", [TINY_QWEN2, TINY_NEOX], ids=lambda c: c.name)
def test_engine_h3_ragged(cfg, B, S):
    """The fp32 HIP engine on windows that are no multiple of any tile, against the fp64 autograd oracle at
    test_relevance_engine_h3_tiny_vs_autograd's 1e-5; window 0 of the batch of 3 equals its B = 1 run bit for bit."""
    from llm_inference_in_distributed_edge_networks_amd.relevance.attnlrp import head_relevance_batched
    from llm_inference_in_distributed_edge_networks_amd.relevance.engine_f32 import RelevanceEngineH3
    mg = DecoderLM.random_init(cfg, 3, device=DEV, std=0.05)
    mc = DecoderLM.random_init(cfg, 3, std=0.05)
    ids = ragged_ids(cfg, B, S)
    eng = RelevanceEngineH3(mg)
    got = eng.head_relevance(ids.to(DEV), want_channels=True, want_sens=True, want_qerr=True)
    torch.cuda.synchronize()
    want = head_relevance_batched(mc, ids, dtype=torch.float64, want_sens=True, want_qerr=True)
    for n, a, b in zip(("rel", "in_rel", "seed", "chan", "sens", "qerr"), got, want):
        e = rel_err(a, b)
        print(f"LRPEDGE engine.h3 {cfg.name} {(B, S)} {n} {e:.3e}")
        assert a.shape == b.shape and e < 1e-5, f"{n}: {e:.3g}"
    if B == 3:
        one = eng.head_relevance(ids[:1].to(DEV), want_channels=True, want_sens=True, want_qerr=True)
        for n, a, b in zip(("rel", "in_rel", "seed", "chan", "sens", "qerr"), got, one):
            assert torch.equal(a[:1], b), f"{n}: window 0 of the batch differs from its own run"


@pytest.mark.parametrize("B,S", RAGGED)
@pytest.mark.parametrize("cfg", [TINY_QWEN2, TINY_NEOX], ids=lambda c: c.name)
def test_engine_bf16_ragged(cfg, B, S):
    """The bf16 HIP engine on the same windows against the fp32 CPU engine on the same (bf16-rounded) weights, at
    test_relevance_engine_gpu_vs_cpu's tolerances."""
    from llm_inference_in_distributed_edge_networks_amd.relevance.engine import RelevanceEngine
    mg = DecoderLM.random_init(cfg, 3, device=DEV, dtype=torch.bfloat16, std=0.05)
    mc = DecoderLM.random_init(cfg, 3, std=0.05)
    for Lg, Lc in zip(mg.layers, mc.layers):
        for kk in Lc:
            Lc[kk] = Lg[kk].float().cpu() if kk in Lg else Lc[kk]
    for kk in ("embed", "head", "norm_w", "norm_b"):
        if mc.w.get(kk) is not None:
            mc.w[kk] = mg.w[kk].float().cpu()
    mc.layers = mc.w["layers"]
    ids = ragged_ids(cfg, B, S)
    top = mc.logits(mc.forward_hidden(ids)).view(B, S, -1)[:, -1].topk(2, -1).values
    assert float(((top[:, 0] - top[:, 1]) / top[:, 0].abs()).min()) > 2e-2, "the seed token is not resolved in bf16"
    rg, ing, mxg = RelevanceEngine(mg).head_relevance(ids.to(DEV))
    rc, inc, mxc = RelevanceEngine(mc).head_relevance(ids)
    wg, wc = rg.sum(0), rc.sum(0)
    e_mx, e_rel = rel_err(mxg, mxc), rel_err(rg, rc)
    e_tab = rel_err(wg / wg.sum(-1, keepdim=True), wc / wc.sum(-1, keepdim=True))
    print(f"LRPEDGE engine.bf16 {cfg.name} {(B, S)} seed {e_mx:.3e} rel {e_rel:.3e} table {e_tab:.3e}")
    assert e_mx < 1e-2 and e_rel < 0.02 and e_tab < 0.04, (e_mx, e_rel, e_tab)
