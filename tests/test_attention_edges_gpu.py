"""The cases of test_attention_edges.py on the HIP kernels: the bf16 and fp32 forward attention families
(csrc/attention.hip, csrc/attention_f32.hip), the importance scorers and head_combine at every length of ``EDGE_S``
(one off the 16-row wave tile, the 64-key tile and the 128-row workgroup; S = 1 and 2), with 6, 9 and 17 (window,
kv head) groups, on rows that drive the online softmax to its corners (``helpers.attention_case``), against fp64;
and ragged windows through whole models in the fp32 and bf16 modes against the CPU fp32 model."""
import math
from functools import lru_cache

import pytest
import torch

import helpers as T
import test_attention_edges as E
from llm_inference_in_distributed_edge_networks_amd import ops
from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows, window_nll
from llm_inference_in_distributed_edge_networks_amd.models import TINY_NEOX, TINY_QWEN2, DecoderLM
from llm_inference_in_distributed_edge_networks_amd.ops import reference as R
from llm_inference_in_distributed_edge_networks_amd.parallel import BoundaryConfig, LocalPipeline, PipelinePlan

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Asserted bounds of the fp32 kernels, per kernel path, output and kind: twice the largest error measured on the
# MI355X over every length and layout of that kind, rounded up to one digit (docs/RESULTS.md section 9: the kernels
# are deterministic, what is left to vary is the compiler), and never above the derived cap ``helpers.edge_caps``.
# Where the measured error is 0 or below one rounding (flat: exact scores; sink150: the probability of key 0 is 1.0)
# the bound is 3e-7 > 2^-22: two fp32 roundings of an output at the scale of max |ref|.  The largest error / cap is
# 0.38 (LSE), 0.23 (column sums) and below 0.07 elsewhere: no kind comes near its cap.
#   x6: three bf16 planes (in_scales=None)     h3: two scaled fp16 planes (in_scales; the KVP kernel is bit-identical)
#   f32: the exact-product importance kernels  h3: the importance kernels on the forward's planes
#   fallback: attn_lastrow with in_scales at G > 16 or G * S * 4 > 60 KiB (the exact kernel)
# f32.colsum is given the fp64 LSE rounded to fp32, so it shows its own fp32 score sums (|s| ~ 150 on sink150: an ulp
# of 1.5e-5 in the exponent); h3.colsum takes the LSE of the forward on the same planes and is self-consistent.
MEASURED_BOUND = {
    "x6.o": {"rand": 4e-06, "flat": 3e-07, "sink30": 9e-06, "sink150": 5e-07, "diag60": 6e-06, "ramp7.5": 7e-06,
             "ramp8": 8e-06, "ramp8.5": 6e-06, "ramp16": 1e-05, "down40": 5e-06},
    "h3.o": {"rand": 6e-06, "flat": 3e-07, "sink30": 7e-06, "sink150": 6e-07, "diag60": 4e-06, "ramp7.5": 5e-06,
             "ramp8": 6e-06, "ramp8.5": 6e-06, "ramp16": 9e-06, "down40": 4e-06},
    "x6.lse": {"rand": 2e-05, "flat": 2e-06, "sink30": 5e-05, "sink150": 2e-04, "diag60": 5e-05, "ramp7.5": 4e-05,
               "ramp8": 5e-05, "ramp8.5": 5e-05, "ramp16": 5e-05, "down40": 2e-05},
    "h3.lse": {"rand": 2e-05, "flat": 3e-06, "sink30": 4e-05, "sink150": 2e-04, "diag60": 4e-05, "ramp7.5": 3e-05,
               "ramp8": 3e-05, "ramp8.5": 3e-05, "ramp16": 4e-05, "down40": 2e-05},
    "f32.lastrow": {"rand": 4e-06, "flat": 3e-07, "sink30": 4e-06, "sink150": 3e-07, "diag60": 4e-06,
                    "ramp7.5": 6e-06, "ramp8": 6e-06, "ramp8.5": 7e-06, "ramp16": 2e-05, "down40": 4e-06},
    "h3.lastrow": {"rand": 4e-06, "flat": 3e-07, "sink30": 4e-06, "sink150": 3e-07, "diag60": 3e-06,
                   "ramp7.5": 5e-06, "ramp8": 4e-06, "ramp8.5": 5e-06, "ramp16": 7e-06, "down40": 3e-06},
    "fallback.lastrow": {"rand": 6e-06, "flat": 3e-07, "sink30": 5e-06, "sink150": 3e-07, "diag60": 7e-06,
                         "ramp7.5": 7e-06, "ramp8": 5e-06, "ramp8.5": 6e-06, "ramp16": 2e-05, "down40": 3e-06},
    "f32.colsum": {"rand": 6e-06, "flat": 4e-07, "sink30": 4e-05, "sink150": 2e-04, "diag60": 7e-05,
                   "ramp7.5": 6e-06, "ramp8": 6e-06, "ramp8.5": 9e-06, "ramp16": 2e-05, "down40": 6e-06},
    "h3.colsum": {"rand": 3e-06, "flat": 6e-07, "sink30": 7e-06, "sink150": 5e-05, "diag60": 2e-05,
                  "ramp7.5": 3e-06, "ramp8": 3e-06, "ramp8.5": 4e-06, "ramp16": 4e-06, "down40": 3e-06},
}


def bound(path, name, kid, caps):
    return min(caps[name], MEASURED_BOUND.get(f"{path}.{name}", {}).get(kid, math.inf))


def check(path, name, kid, layout, S, got, ref, caps, yard):
    """Print the measured error (and its ratio to the CPU fp32 oracle's own error on the case), then assert."""
    err = T.edge_err(name, got, ref[name])
    y = T.edge_err(name, yard[name], ref[name])
    print(f"EDGE {path}.{name} {kid} {layout} S={S} err {err:.3e} cap {caps[name]:.3e} oracle {y:.3e} "
          f"ratio {err / max(y, 1e-30):.2f}")
    b = bound(path, name, kid, caps)
    assert err <= b, (path, name, kid, layout, S, err, b)


def close(a, b, atol, rtol):
    a, b = a.double().cpu().reshape(b.shape), b.double()
    assert torch.isfinite(a).all(), "non-finite output"
    err = (a - b).abs()
    assert (err <= atol + rtol * b.abs()).all(), f"max err {err.max().item():.4g} (atol {atol}, rtol {rtol})"


@lru_cache(maxsize=8)
def bf16_ref(kid, layout, S):
    """The bf16-rounded inputs and the fp64 reference on them (what the bf16 kernels are held to)."""
    q, k, v = (t.bfloat16() for t in E.edge_ref(kid, layout, S)[:3])
    ref = dict(zip(E.OUTPUTS, T.attention_all64(q.float(), k.float(), v.float(), S)))
    return q, k, T.vt_of(v, S), ref


def scales(q, k, v):
    """in_scales of the fp16-plane kernels from the case's own maxima: powers of two with s |x| <= 2^15."""
    return tuple(R.h3_scale(float(t.abs().max())) for t in (q, k, v))


def forwards(kid, layout, S, n_rows=None):
    """The four forwards: (a) bf16, (b) fp32 on three bf16 planes, (c) fp32 on fp16 planes (fp32 rows and h3 output),
    (d) the LDS-DMA plane kernel with h3 output and fp32 side output."""
    q, k, v, vt = E.edge_ref(kid, layout, S)[:4]
    qb, kb, vtb, _ = bf16_ref(kid, layout, S)
    sc = scales(q, k, v)
    s = sc[2]                                                     # |o| <= max |v|
    kp, vp = R.kv_planes(k, vt, sc[1], sc[2])
    qd, kd, vtd = q.to(DEV), k.to(DEV), vt.to(DEV)
    nr = None if n_rows is None else n_rows.to(DEV)
    out = {"a": ops.attention(qb.to(DEV), kb.to(DEV), vtb.to(DEV), S, need_lse=True, n_rows=nr),
           "b": ops.attention(qd, kd, vtd, S, need_lse=True, n_rows=nr),
           "c": ops.attention(qd, kd, vtd, S, need_lse=True, n_rows=nr, in_scales=sc),
           "c3": ops.attention(qd, kd, vtd, S, need_lse=True, n_rows=nr, in_scales=sc, h3=s),
           "d": ops.attention(qd, None, None, S, need_lse=True, n_rows=nr, in_scales=sc, h3=s,
                              kv_planes=(kp.to(DEV), vp.to(DEV)), f32_out=True)}
    torch.cuda.synchronize()
    return out, s


@pytest.mark.parametrize("S", T.EDGE_S)
@pytest.mark.parametrize("kid", T.EDGE_KIND_IDS)
def test_forward(kid, S):
    for layout in T.EDGE_LAYOUTS:
        ref, caps, yard = E.edge_ref(kid, layout, S)[4:]
        f, s = forwards(kid, layout, S)
        o3, lse_d, o32 = f["d"]
        # 1. the plane-staged kernel equals the kernel that splits fp32 K / V^T itself, bit for bit
        assert torch.equal(o3, f["c3"][0]) and torch.equal(lse_d, f["c3"][1]), (layout, "h3 planes / LSE")
        assert torch.equal(o32, f["c"][0]) and torch.equal(lse_d, f["c"][1]), (layout, "fp32 rows / LSE")
        # 2. the h3 planes are the split of the fp32 side output
        assert torch.equal(o3, ops.split_h3(o32, s)), layout
        # 3. finite everywhere
        for key, outs in f.items():
            assert all(torch.isfinite(t.float()).all() for t in outs), (layout, key)
        # 4. against fp64
        for path, key in (("x6", "b"), ("h3", "c")):
            check(path, "o", kid, layout, S, f[key][0], ref, caps, yard)
            check(path, "lse", kid, layout, S, f[key][1], ref, caps, yard)
        rb = bf16_ref(kid, layout, S)[3]
        close(f["a"][0], rb["o"], atol=3e-2, rtol=2e-2)            # test_flash_attention_spike's tolerances
        close(f["a"][1], rb["lse"], atol=1e-2, rtol=1e-3)


@pytest.mark.parametrize("S", [129, 257])
@pytest.mark.parametrize("kid", T.EDGE_KIND_IDS)
def test_forward_scored_rows(kid, S):
    """Scored-rows mode (the model's last layer): only the last 128-row block, one row into the block before it, and
    everything; the rows >= S - 1 - n_rows[b] equal the full run's bit for bit, output and LSE, in every forward."""
    for layout in T.EDGE_LAYOUTS:
        B, Hq, _ = layout
        n_rows = torch.tensor([float((0, 1, S - 1)[b % 3]) for b in range(B)])
        full, _ = forwards(kid, layout, S)
        part, _ = forwards(kid, layout, S, n_rows)
        for key in full:
            for t_full, t_part in zip(full[key], part[key]):
                rows = t_full.dim() == 2                            # o [B * S, W] (lse: [B, Hq, S])
                a = t_full.view(B, S, -1) if rows else t_full
                c = t_part.view(B, S, -1) if rows else t_part
                for b in range(B):
                    lo = S - 1 - int(n_rows[b])
                    same = torch.equal(a[b, lo:], c[b, lo:]) if rows else torch.equal(a[b, :, lo:], c[b, :, lo:])
                    assert same, (layout, key, b, "rows" if rows else "lse")


@pytest.mark.parametrize("S", T.EDGE_S)
@pytest.mark.parametrize("kid", T.EDGE_KIND_IDS)
def test_importance(kid, S):
    for layout in E.LAYOUTS:                                        # with G = 16, the full tile of attn_lastrow_h3
        q, k, v, vt, ref, caps, yard = E.edge_ref(kid, layout, S)
        qb, kb, vtb, rb = bf16_ref(kid, layout, S)
        qd, kd = q.to(DEV), k.to(DEV)
        sc = scales(q, k, v)
        # bf16 (test_importance_kernels' tolerances): the column sums from the LSE of the bf16 forward
        qbd, kbd = qb.to(DEV), kb.to(DEV)
        _, lse_b = ops.attention(qbd, kbd, vtb.to(DEV), S, need_lse=True)
        close(ops.attn_lastrow(qbd, kbd, S), rb["lastrow"], atol=1e-4, rtol=2e-3)
        close(ops.attn_colsum(qbd, kbd, lse_b, S), rb["colsum"], atol=2e-3, rtol=5e-3)
        # fp32, exact products: the column sums from the reference LSE rounded to fp32
        check("f32", "lastrow", kid, layout, S, ops.attn_lastrow(qd, kd, S), ref, caps, yard)
        check("f32", "colsum", kid, layout, S, ops.attn_colsum(qd, kd, ref["lse"].float().to(DEV), S), ref, caps,
              yard)
        # fp32 on the forward's fp16 planes: the column sums from the LSE that forward wrote, as the model does
        _, lse_c = ops.attention(qd, kd, vt.to(DEV), S, need_lse=True, in_scales=sc)
        check("h3", "lastrow", kid, layout, S, ops.attn_lastrow(qd, kd, S, in_scales=sc[:2]), ref, caps, yard)
        check("h3", "colsum", kid, layout, S, ops.attn_colsum(qd, kd, lse_c, S, in_scales=sc[:2]), ref, caps, yard)


# attn_lastrow with in_scales falls back to the exact kernel when the G score rows do not fit the MFMA tile (G > 16)
# or the 60 KiB of LDS (G * S * 4 bytes): G = 32, and G = 8 at S = 2048 (64 KiB)
@pytest.mark.parametrize("kid,B,Hq,Hkv,S", [(kid, 1, 32, 1, S) for kid in T.EDGE_KIND_IDS for S in (1, 65, 257)]
                         + [(kid, 1, 8, 1, 2048) for kid in ("rand", "flat", "sink150")])
def test_lastrow_fallbacks(kid, B, Hq, Hkv, S):
    kind, amp = T.EDGE_KIND[kid]
    q, k, v = T.attention_case(kind, B, Hq, Hkv, S, amp, T.edge_seed(B, Hq, Hkv, S))
    ref = R.attn_lastrow(q.double(), k.double(), S)
    cap = 2e-6 + 4 * T.score_eps(q, k, S)
    sc = scales(q, k, v)
    got = ops.attn_lastrow(q.to(DEV), k.to(DEV), S, in_scales=sc[:2])
    err, y = T.edge_err("lastrow", got, ref), T.edge_err("lastrow", R.attn_lastrow(q, k, S), ref)
    print(f"EDGE fallback.lastrow {kid} {(B, Hq, Hkv)} S={S} err {err:.3e} cap {cap:.3e} oracle {y:.3e} "
          f"ratio {err / max(y, 1e-30):.2f}")
    assert torch.isfinite(ref).all() and err <= bound("fallback", "lastrow", kid, {"lastrow": cap})


@pytest.mark.parametrize("B,S", [(1, 1), (3, 257), (2, 128)])
def test_head_combine(B, S):
    """out = beta out + scale sum_h w[h] x[:, h]: without weights, with beta = 0 into a NaN-filled buffer (which must
    be ignored, not multiplied by 0), and accumulating (aggregate_till's running sum) - a length-Hq fp32 sum, held to
    1e-6 of max |ref|."""
    Hq = 14
    g = torch.Generator().manual_seed(90 + S)
    x, w, acc = torch.randn(B, Hq, S, generator=g), torch.randn(Hq, generator=g), torch.randn(B, S, generator=g)
    xd, wd = x.to(DEV), w.to(DEV)

    def want(wv, scale, out=None, beta=0.0):
        r = scale * (x.double() * wv.double().view(1, -1, 1)).sum(1)
        return r if out is None else beta * out.double() + r

    def ok(got, ref):
        assert got.shape == (B, S) and T.edge_err("o", got, ref) <= 1e-6

    ok(ops.head_combine(xd), want(torch.ones(Hq), 1.0))
    ok(ops.head_combine(xd, None, 1.0 / S), want(torch.ones(Hq), 1.0 / S))
    ok(ops.head_combine(xd, wd, 0.25), want(w, 0.25))
    nan = torch.full((B, S), float("nan"), device=DEV)
    got = ops.head_combine(xd, wd, 0.25, out=nan, beta=0.0)
    assert got.data_ptr() == nan.data_ptr()
    ok(got, want(w, 0.25))
    for beta in (1.0, 0.5):
        for wv, wr in ((wd, w), (None, torch.ones(Hq))):
            out = acc.to(DEV)
            ok(ops.head_combine(xd, wv, 1.0 / S, out=out, beta=beta), want(wr, 1.0 / S, acc, beta))


# ---- ragged windows through whole models ---------------------------------------------------------------------
def ragged_batches():
    """The last three batches of a 2997-token stream at length 256, stride 32, batch 4 - (4, 256), (2, 256) and the
    ragged last window (1, 245) with 21 scored rows - and a 77-token stream's single window (76 scored rows)."""
    t1, t2 = synthetic_stream(2997, 512, 4), synthetic_stream(77, 512, 4)
    return (list(batches(t1, sliding_windows(2997, 256, 32), 4))[-3:]
            + list(batches(t2, sliding_windows(77, 256, 32), 4)))


def model_rows(m, b):
    b = b.to(m.device)
    return m.row_nll(m.forward_hidden(b.ids), b.rows, b.targets)


def model_nll(m, b):
    return window_nll(model_rows(m, b), b.to(m.device)).double().cpu()


@lru_cache(maxsize=None)
def cpu_nll(name):
    """Per-window NLL of the CPU fp32 model on every ragged batch, and its one-split pipeline's (no quantisation)."""
    cfg = {"qwen2": TINY_QWEN2, "neox": TINY_NEOX}[name]
    m = DecoderLM.random_init(cfg, 3, device="cpu", dtype=torch.float32, std=0.05)
    pipe = LocalPipeline(m, PipelinePlan.from_split_layers(cfg.num_layers, [1]), BoundaryConfig())
    bl = ragged_batches()
    return (cfg, [model_nll(m, b) for b in bl], [pipe.run_batch(b).double() for b in bl], pipe.evaluate(bl).ppl(),
            [model_rows(m, b).double() for b in bl])


@pytest.mark.parametrize("name", ["qwen2", "neox"])
def test_ragged_windows_fp32(name):
    """fp32 mode (the default precision) on ragged windows: per-window NLL within 1e-4 relative of the CPU fp32 model
    (test_full_model_nll_matches_cpu_fp32's bound), directly and through a one-split pipeline without quantisation,
    whose captured graph equals eager bit for bit on every batch."""
    cfg, want, want_pipe, want_ppl, _ = cpu_nll(name)
    bl = ragged_batches()
    assert [tuple(b.ids.shape) for b in bl] == [(4, 256), (2, 256), (1, 245), (1, 77)]
    m = DecoderLM.random_init(cfg, 3, device=DEV, dtype=torch.float32, std=0.05)
    for b, w in zip(bl, want):
        got = model_nll(m, b)
        rel = ((got - w).abs() / w.abs()).max().item()
        print(f"EDGE model {name} fp32 {tuple(b.ids.shape)} rel {rel:.2e}")
        assert rel < 1e-4, (tuple(b.ids.shape), rel)
    plan = PipelinePlan.from_split_layers(cfg.num_layers, [1])
    eager = LocalPipeline(m, plan, BoundaryConfig(), use_graphs=False)
    graphed = LocalPipeline(m, plan, BoundaryConfig(), use_graphs=True)
    dl = [b.to(DEV) for b in bl]
    for it in range(3):                                             # eager warm-up, capture, replay
        for b, w in zip(dl, want_pipe):
            e, g = eager.run_batch(b).clone(), graphed.run_batch(b).clone()
            assert torch.equal(e, g), (it, tuple(b.ids.shape))
            assert ((e.double().cpu() - w).abs() / w.abs()).max().item() < 1e-4
    assert graphed.graphs.graphs, "nothing was captured"
    for pipe in (eager, graphed):
        ppl = pipe.evaluate(bl).ppl()
        assert abs(ppl - want_ppl) / want_ppl < 1e-4, (ppl, want_ppl)


@pytest.mark.parametrize("name", ["qwen2", "neox"])
def test_ragged_windows_bf16(name):
    """bf16 mode on the same batches: test_tiny_model_gpu_vs_cpu's criterion (mean |row NLL difference| below 5 % of
    the mean row NLL + 1e-2), per window."""
    cfg, _, _, _, want_rows = cpu_nll(name)
    m = DecoderLM.random_init(cfg, 3, device=DEV, dtype=torch.bfloat16, std=0.05)
    for b, w in zip(ragged_batches(), want_rows):
        got = model_rows(m, b).double().cpu()
        assert torch.isfinite(got).all()
        for i, (gw, ww) in enumerate(zip(got.split(b.n_rows.int().tolist()), w.split(b.n_rows.int().tolist()))):
            d, ref = float((gw - ww).abs().mean()), float(ww.abs().mean())
            print(f"EDGE model {name} bf16 {tuple(b.ids.shape)} window {i} mean |dNLL| {d:.2e} of {ref:.2f}")
            assert d < 0.05 * ref + 1e-2, (tuple(b.ids.shape), i, d, ref)
