"""Batched AttnLRP head relevance on the framework's own kernels.

Same quantity as ``attnlrp.head_relevance`` (the reference's ``Relevance/main.py:84-103``: seed the max
logit of the last position with its own value, backpropagate with the AttnLRP rules, sum ``A * dA`` per
head), computed without autograd and without any S x S tensor:

* forward with saves: the regular fused layer kernels (QKV+RoPE with the RMSNorm row scale folded in,
  flash attention with its row LSE, O / gate-up / down GEMMs), keeping q, k, v, o, lse, the gate|up
  pre-activations and the norm row scales of every layer;
* seed: only the B last rows carry gradient (``d hN = mx * W_head[argmax]``, detached final norm), so the last
  layer runs its O projection and MLP on those rows only, forward and backward;
* backward per layer, in reverse: input-gradient GEMMs with the transposed weights (norm row scale and
  residual in the epilogue), the SwiGLU / GELU / LayerNorm rules, and the attention backward kernel
  (``csrc/lrp.hip``) that also emits the per-(window, head) relevance ``0.5 sum_i dO_i . O_i``.

CUDA tensors run the gfx950 kernels (bf16 storage, fp32 accumulation); CPU tensors run the fp32 reference
ops, which the tests check against the autograd oracle.  Windows of one batch are independent, so a
batch of B windows gives B relevance tables in one pass.
"""
from __future__ import annotations


import torch

from .. import ops
from ..ops import reference as R
from ..models.model import DecoderLM


class RelevancePass:
    """The pass both engines run: forward with saves, seed on the last row of each window, the reverse layer loop and
    the per-layer tables.  An engine supplies ``_layer_weights`` (the backward GEMMs' weights of one layer),
    ``_forward``, ``_seed``, ``_backward_layer``, ``_tables`` and ``_input_relevance``."""
    # ``_tables`` fills chan and sens in one kernel over 64-channel groups: no other group width, and the chan table
    # exists whenever sens is wanted
    fused_tables = False

    def __init__(self, model: DecoderLM):
        self.m = model
        cfg = model.cfg
        if cfg.head_dim != 64:
            raise ValueError("relevance engine is specialised for head_dim 64")
        if any(L is None for L in model.layers) or model.w.get("embed") is None or model.w.get("head") is None:
            raise ValueError("relevance engine needs the whole model resident")
        self.qwen = cfg.arch == "qwen2"
        self.T = [self._layer_weights(L) for L in model.layers]

    @staticmethod
    def _to_all_rows(rows: torch.Tensor, n: int, *ts):
        """The last layer's gradients at the seeded rows ``rows`` -> at all ``n`` rows, zero elsewhere."""
        return [None if t is None else
                torch.zeros(n, t.shape[1], dtype=t.dtype, device=t.device).index_copy_(0, rows, t) for t in ts]

    @torch.no_grad()
    def head_relevance(self, ids: torch.Tensor, want_channels: bool = False, group: int = 64,
                       want_sens: bool = False, want_qerr: bool = False):
        """ids [B, S] (B windows of equal length) -> (rel [B, layers, heads] fp32, input relevance [B],
        seed logit [B][, chan [B, layers, H / group]][, sens [B, layers, H / group]][, qerr [B, layers, H / 64, 2,
        6]]: ``want_qerr``, the groups' measured quantization error, ``ops.group_quant_err``).  rel[b, l, h] = sum_{i,j}
        A_ij dA_ij of head h, layer l, window b; chan (``want_channels``) = sum over tokens and the group's channels
        of |x * dx| of the residual stream entering layer l (as ``attnlrp.head_relevance_batched``); sens
        (``want_sens``) = the groups' quantization sensitivity (``ops.reference.group_sens``)."""
        if group != 64 and self.fused_tables:
            raise ValueError("channel groups are 64 channels (one head) wide")
        if group != 64 and want_qerr:
            raise ValueError("the measured quantization error is of 64-channel groups")
        m, cfg = self.m, self.m.cfg
        ids = ids.to(m.device)
        B, S = ids.shape
        H = cfg.hidden_size
        emb, x, saves = self._forward(ids)
        dx, mx = self._seed(x, B, S)   # x, dx: the seeded rows only [B, H] (the last layer's ``rows``)

        def table(want, *shape):
            return torch.zeros(B, cfg.num_layers, *shape, dtype=torch.float32, device=m.device) if want else None
        rel = table(True, cfg.num_heads)
        chan = table(want_channels or (want_sens and self.fused_tables), H // group)
        sens = table(want_sens, H // group)
        qerr = table(want_qerr, H // 64, 2, 6)
        for i in range(cfg.num_layers - 1, -1, -1):
            sv = saves[i]
            rel[:, i], dx = self._backward_layer(i, dx, sv)
            self._tables(i, sv["x"], dx, B, S, group, chan, sens, qerr)
            saves[i] = None
        in_rel = self._input_relevance(emb, dx, B, S)
        return (rel, in_rel, mx) + ((chan,) if want_channels else ()) + ((sens,) if want_sens else ()) \
            + ((qerr,) if want_qerr else ())


class RelevanceEngine(RelevancePass):
    def _layer_weights(self, L: dict) -> dict:
        """Transposed / norm-folded weights of one layer's backward GEMMs."""
        if not self.qwen:
            return dict(wqkvT=L["wqkv"].t().contiguous(), woT=L["wo"].t().contiguous(),
                        wfcT=L["wfc"].t().contiguous(), wprojT=L["wproj"].t().contiguous())
        wqkv_n = L.get("wqkv_n")
        wgu_n = L.get("wgu_n")
        if wqkv_n is None:
            wqkv_n = ops.reference.fold_norm_weight(L["wqkv"], L["ln1_w"]).contiguous()
            wgu_n = ops.reference.fold_norm_weight(L["wgu"], L["ln2_w"]).contiguous()
        return dict(wqkv_n=wqkv_n, wgu_n=wgu_n, wqkvT=wqkv_n.t().contiguous(), woT=L["wo"].t().contiguous(),
                    wguT=wgu_n.t().contiguous(), wdT=L["wd"].t().contiguous())

    # ------------------------------------------------------------------------------------------------
    def _forward(self, ids: torch.Tensor):
        # The with-saves sequence, kept apart from ``DecoderLM.layer`` (and from the fp32 engine's) on purpose: it
        # launches different kernels - ``row_ssq`` + ``row_rscale`` per layer, the raw-emitting SwiGLU GEMM, no
        # ``want_ssq`` on the down GEMM - and a ``save=`` switch would put those branches into the hot forward.
        m, cfg = self.m, self.m.cfg
        B, S = ids.shape
        H, Hq, Hkv, D = cfg.hidden_size, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim
        x = m.embed(ids)
        emb = x
        saves = []
        last = torch.arange(B, device=ids.device) * S + (S - 1)   # the seeded rows
        nl = len(m.layers)
        for i, L in enumerate(m.layers):
            t = self.T[i]
            sv = {"x": x}
            if self.qwen:
                ssq1 = ops.row_ssq(x)
                sv["rs1"] = ops.row_rscale(ssq1, H, cfg.norm_eps)
                q, k, vt = ops.qkv_rope(x, t["wqkv_n"], L["bqkv"], m.cos, m.sin, B, S, Hq, Hkv, D, cfg.rotary_dim,
                                        m.q_scale, norm=(ssq1, cfg.norm_eps))
            else:
                sv["rs1"] = ops.ln_rstd(x, cfg.norm_eps)
                h1, h2 = ops.layernorm_dual(x, L["ln1_w"], L["ln1_b"], L["ln2_w"], L["ln2_b"], cfg.norm_eps)
                q, k, vt = ops.qkv_rope(h1, L["wqkv"], L["bqkv"], m.cos, m.sin, B, S, Hq, Hkv, D, cfg.rotary_dim,
                                        m.q_scale)
            o, lse = ops.attention(q, k, vt, S, need_lse=True)
            sv.update(q=q, k=k, v=vt[..., :S].transpose(-1, -2).contiguous(), o=o, lse=lse.contiguous())
            if i == nl - 1:   # only the seeded rows reach the seed: O-proj and MLP on those rows
                sv["rows"] = last
                o, x = o.index_select(0, last), x.index_select(0, last)
                if not self.qwen:
                    h2 = h2.index_select(0, last)
            if self.qwen:
                y = ops.linear(o, L["wo"], residual=x, want_ssq=True)
                ssq2 = y._edge_ssq
                sv["rs2"] = ops.row_rscale(ssq2, H, cfg.norm_eps)
                # one GEMM: the SwiGLU activation and the saved pre-activations for its rule
                a, sv["gu"] = ops.linear_swiglu_raw(y, t["wgu_n"], norm=(ssq2, cfg.norm_eps))
                x = ops.linear(a, L["wd"], residual=y)
            else:
                a = ops.linear(h2, L["wfc"], L["bfc"])
                sv["a"] = a
                f = ops.linear(h2, L["wfc"], L["bfc"], act="gelu")
                y = ops.linear(o, L["wo"], L["bo"], residual=x)
                x = ops.linear(f, L["wproj"], L["bproj"], residual=y)
            saves.append(sv)
        return emb, x, saves

    def _seed(self, x: torch.Tensor, B: int, S: int):
        """Gradient of ``mx * mx`` w.r.t. the final hidden state (x: the last row of each window, [B, H]) -> (the
        seed gradient [B, H], the seed logits)."""
        m, cfg = self.m, self.m.cfg
        last = x.float()
        w = m.w["norm_w"].float()
        if self.qwen:
            rstd = torch.rsqrt(last.pow(2).mean(-1, keepdim=True) + cfg.norm_eps)
            hN = last * rstd * w
        else:
            xc = last - last.mean(-1, keepdim=True)
            rstd = torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + cfg.norm_eps)
            hN = xc * rstd * w + m.w["norm_b"].float()
        head = m.w["head"]
        logits = hN @ head.float().t() if head.device.type == "cpu" else (hN.to(head.dtype) @ head.t()).float()
        mx, idx = logits.max(-1)
        dhN = mx.view(-1, 1) * head.index_select(0, idx).float()
        g = dhN * rstd * w
        if not self.qwen:
            g = g - g.mean(-1, keepdim=True)
        return g.to(x.dtype).contiguous(), mx

    def _backward_layer(self, i: int, dx: torch.Tensor, sv: dict):
        m, cfg = self.m, self.m.cfg
        L, t = m.layers[i], self.T[i]
        B, Hq, S, _ = sv["q"].shape
        dh2 = None
        if self.qwen:
            dm = ops.linear(dx, t["wdT"])
            dy = ops.linear_rowscale(ops.lrp_swiglu_bwd(dm, sv["gu"]), t["wguT"], sv["rs2"], residual=dx)
        else:
            dh2 = ops.linear(ops.lrp_gelu_bwd(ops.linear(dx, t["wprojT"]), sv["a"]), t["wfcT"])
            dy = dx
        dO = ops.linear(dy, t["woT"])
        if "rows" in sv:   # last layer: dx is the seeded rows only [B, H]
            dO, dy, dh2 = self._to_all_rows(sv["rows"], B * S, dO, dy, dh2)
        _, r, dq, dk, dv = ops.lrp_attn_bwd(sv["q"], sv["k"], sv["v"], sv["o"], dO, sv["lse"])
        dqkv = ops.lrp_rope_pack(dq, dk, dv, m.cos, m.sin, B, S, Hq, cfg.num_kv_heads, cfg.rotary_dim, m.q_scale,
                                 dtype=dx.dtype)
        if self.qwen:
            return r, ops.linear_rowscale(dqkv, t["wqkvT"], sv["rs1"], residual=dy)
        dh1 = ops.linear(dqkv, t["wqkvT"])
        return r, ops.lrp_ln_bwd(dh1, sv["rs1"], L["ln1_w"], dh2, sv["rs1"], L["ln2_w"], dy)

    def _tables(self, i, x, dx, B, S, group, chan, sens, qerr):
        if chan is not None:
            chan[:, i] = (x.float() * dx.float()).abs().view(B, S, -1, group).sum((1, 3))
        if sens is not None:
            sens[:, i] = R.group_sens(x, dx, B, S, group)
        if qerr is not None:
            qerr[:, i] = ops.group_quant_err(x.contiguous(), dx.float().contiguous(), B, S)

    def _input_relevance(self, emb, dx, B, S):
        return (emb.float() * dx.float()).view(B, S, -1).sum((1, 2))
