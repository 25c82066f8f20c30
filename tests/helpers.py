import torch

from llm_inference_in_distributed_edge_networks_amd.models import DecoderLM


def hf_qwen2(cfg, seed=0):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(seed)
    hc = Qwen2Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                     num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                     num_key_value_heads=cfg.num_kv_heads, max_position_embeddings=cfg.max_position,
                     rope_theta=cfg.rope_theta, tie_word_embeddings=cfg.tie_embeddings, rms_norm_eps=cfg.norm_eps,
                     attn_implementation="eager")
    m = Qwen2ForCausalLM(hc).eval()
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("bias"):
                v.normal_(0, 0.1)
            elif "norm" in k:
                v.normal_(1, 0.1)
    return m


def hf_neox(cfg, seed=0):
    from transformers import GPTNeoXConfig, GPTNeoXForCausalLM
    torch.manual_seed(seed)
    hc = GPTNeoXConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
                       intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_layers,
                       num_attention_heads=cfg.num_heads, rotary_pct=cfg.rotary_dim / cfg.head_dim,
                       max_position_embeddings=cfg.max_position, layer_norm_eps=cfg.norm_eps,
                       attn_implementation="eager", hidden_act="gelu", tie_word_embeddings=False)
    m = GPTNeoXForCausalLM(hc).eval()
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("bias"):
                v.normal_(0, 0.1)
    return m


def ours_from_hf(cfg, hf):
    return DecoderLM.from_state_dict(cfg, hf.state_dict())


# ---- variable-k (top-rho) boundary messages: inputs on which the CPU codec and the HIP kernels agree bit for bit ---
KVAR_CODECS = ["ref_int4_global", "int4_token", "mixed_int4_int8", "mixed_int2_int8", "int8_token_keep",
               "mixed_mxfp4_mxfp8", "mxfp4_keep", "mixed_rgroup_int8"]      # every codec with spec.uses_ratio
KVAR_RATIOS = [0.25, 0.5, 0.75]                      # keep mass 1 - ratio is exact in fp32
# (B, S, H): partial last workgroup and several windows; B > 64 (second trip of the k-vector reduction), B * S no
# multiple of the four rows per workgroup, half-used mask words, H = 128; S one full mask word pair
KVAR_SHAPES = [(5, 200, 896), (70, 37, 128), (3, 64, 896)]
# non-uniform head-group plans whose row size (8 * sum(bits) + 4 per group) is no multiple of 16
KVAR_GROUP_PLANS = {128: (2, 4), 896: (2, 3, 4, 5, 6, 8, 2, 3, 4, 5, 6, 8, 4, 8)}


def kvar_spec(name, H):
    """The codec under test; the head-group codec with a non-uniform plan."""
    from llm_inference_in_distributed_edge_networks_amd.codec import wire as W
    spec = W.get_codec(name)
    return W.with_plan(spec, KVAR_GROUP_PLANS[H]) if W.needs_plan(spec) else spec


def kvar_seed(B, S):
    return 1000 * B + S


def dyadic_importance(B, S, seed):
    """Token importance [B, S] (fp32) whose top-rho cut is the same in any precision and summation order.

    Every value is n / 65536 with n an integer below 1.8 * 65536 / S, so every partial sum of a window is a multiple
    of 2^-16 below 4: at most 18 significant bits, exact in fp32 whatever the order (the kernel's block scan, the
    oracle's fp64 sequential sums).  With a keep mass that is exact in fp32 (1 - ratio for ratio 0.25 / 0.5 / 0.75)
    the comparison against the threshold is exact as well, so k needs no tolerance.  The windows hold exact ties
    (column 7i + 1 copied into column 7i), one all-zero column, a window 0 of total mass below 0.25 (values below
    40 / 65536, S <= 400: k = 0 at every keep mass >= 0.25) and one token of mass 0.5 in window 1 (k = S - 1 at every
    keep mass <= 0.5)."""
    assert B >= 2 and 8 <= S <= 400
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(0, int(1.8 * 65536 / S), (B, S), generator=g)
    n[0] = torch.randint(0, 40, (S,), generator=g)
    n[1, 3] = 2 ** 15
    for c in range(0, S - 1, 7):
        n[:, c] = n[:, c + 1]
    n[:, 5] = 0
    return (n.double() / 65536).float()


def kvar_activations(B, S, H, seed, dtype=torch.float32):
    """Boundary activations [B * S, H]: randn * 3, one outlier row (x 40, in window 1) and one all-zero row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * S, H, generator=g) * 3
    x[S + 5] *= 40
    x[(B * S) // 2 + 1] = 0
    return x.to(dtype)


# ---- attention / importance kernels on ragged windows and hard softmax rows (test_attention_edges*.py) -------------
# one off the 16-row wave tile, the 64-key tile and the 128-row workgroup, and the shortest windows
EDGE_S = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257]
# (B, Hq, Hkv): B * Hkv = 6, 9, 17 (window, kv head) groups - below 8 (idle XCDs), just above 8 (one XCD owns two
# groups: grp = xcd + 8 * (rem / G)) and above 16 (three)
EDGE_LAYOUTS = [(3, 4, 2), (9, 2, 1), (17, 1, 1)]
EDGE_LAYOUT_G16 = (1, 16, 1)          # G = 16: the full MFMA tile of attn_lastrow_h3
# (id, kind, amp): the structure sits in channel 3, the other channels stay random
EDGE_KINDS = [("rand", "rand", 0.0), ("flat", "flat", 0.0), ("sink30", "sink", 30.0), ("sink150", "sink", 150.0),
              ("diag60", "diag", 60.0), ("ramp7.5", "ramp", 7.5), ("ramp8", "ramp", 8.0), ("ramp8.5", "ramp", 8.5),
              ("ramp16", "ramp", 16.0), ("down40", "down", 40.0)]
EDGE_KIND = {i: (kind, amp) for i, kind, amp in EDGE_KINDS}
EDGE_KIND_IDS = [i for i, _, _ in EDGE_KINDS]
LN2 = 0.6931471805599453


# A dropped last key shows only where some head's last row puts visible mass on its own key, which a random row of
# 128 or more keys may not: these (layout, S) take the first seed of the sequence base + 100000 t on which the
# ``rand`` case meets test_attention_edges.py::test_detection with a margin of two (searched once, asserted there).
EDGE_SEED_STEP = {((3, 4, 2), 64): 1, ((17, 1, 1), 64): 2, ((9, 2, 1), 127): 2, ((1, 16, 1), 127): 1,
                  ((3, 4, 2), 128): 1, ((9, 2, 1), 128): 2, ((1, 16, 1), 128): 2, ((3, 4, 2), 129): 4,
                  ((9, 2, 1), 129): 5, ((1, 16, 1), 129): 4, ((3, 4, 2), 255): 6, ((9, 2, 1), 255): 4,
                  ((17, 1, 1), 255): 1, ((1, 16, 1), 255): 1, ((3, 4, 2), 257): 4, ((17, 1, 1), 257): 9,
                  # S = 31 is a length of the AttnLRP cases only (LRP_EDGE_S): the first seed on which the ``rand``
                  # case meets test_lrp_edges.py::test_detection with a margin of two
                  ((9, 2, 1), 31): 1}


def edge_seed(B, Hq, Hkv, S):
    return 7000 + 1000 * B + 100 * Hq + S + 100000 * EDGE_SEED_STEP.get(((B, Hq, Hkv), S), 0)


def attention_case(kind, B, Hq, Hkv, S, amp, seed):
    """fp32 (q [B, Hq, S, 64] pre-scaled, k, v [B, Hkv, S, 64]) from test_attention_f32's distribution (q = randn / 2,
    k = 2 randn, v = randn), with one structure on top:

    rand  unchanged: tails and masks.
    flat  q = 0: a uniform softmax, o_i = mean(v_0 .. v_i), lse_i = log(i + 1), no cancellation to hide behind.
    sink  q[..., 3] = 1, k[..., 3] = 0, k[:, :, 0, 3] = amp nats: key 0 dominates every row; at amp = 150
          (> 126 ln 2) every later key underflows.
    diag  k_j = amp q_j / |q_j|^2 of the group's first q head: q_j . k_j = amp, every new tile raises the row
          maximum and the rescale factor alpha goes to 0.
    ramp  q[..., 3] = 1, k[..., j, 3] = (j // 64) amp ln 2: the maximum rises by amp (log2 units) per key tile -
          just under, at, just over and at twice the lazy-rescale threshold 8.
    down  ramp with the sign flipped: the maximum sits in tile 0, the tail underflows."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, S, 64, generator=g) * 0.5
    k = torch.randn(B, Hkv, S, 64, generator=g) * 2
    v = torch.randn(B, Hkv, S, 64, generator=g)
    if kind == "rand":
        pass
    elif kind == "flat":
        q.zero_()
    elif kind == "sink":
        q[..., 3] = 1.0
        k[..., 3] = 0.0
        k[:, :, 0, 3] = amp
    elif kind == "diag":
        q0 = q[:, ::Hq // Hkv]
        k = amp * q0 / q0.pow(2).sum(-1, keepdim=True)
    elif kind in ("ramp", "down"):
        q[..., 3] = 1.0
        step = (torch.arange(S) // 64).float() * float(amp * LN2)
        k[..., 3] = step if kind == "ramp" else -step
    else:
        raise ValueError(kind)
    return q.contiguous(), k.contiguous(), v.contiguous()


def edge_case(kid, B, Hq, Hkv, S):
    kind, amp = EDGE_KIND[kid]
    return attention_case(kind, B, Hq, Hkv, S, amp, edge_seed(B, Hq, Hkv, S))


def vt_of(v, S):
    """V [B, Hkv, S, 64] -> V^T [B, Hkv, 64, s_pad] with zero key padding (the attention kernels' layout)."""
    from llm_inference_in_distributed_edge_networks_amd.ops import reference as R
    vt = torch.zeros(*v.shape[:2], 64, R.s_pad(S), dtype=v.dtype)
    vt[..., :S] = v.transpose(-1, -2)
    return vt


def attention_all64(q, k, v, S, shift=0, pad_last=False):
    """fp64 (o [B*S, Hq*64], lse, last row, column sums [B, Hq, S]) from one explicit probability matrix, with the
    mask as a parameter: query i sees keys j <= i + shift (row 0 always keeps key 0); ``pad_last`` hides key S - 1
    from every row as if it were padding.  shift = 0, pad_last = False is the causal attention; the other settings
    are the wrong answers an off-by-one tail or mask would give (the detection check of test_attention_edges.py)."""
    B, Hq = q.shape[:2]
    G = Hq // k.shape[1]
    kk, vv = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    sc = q.double() @ kk.transpose(-1, -2)
    i, j = torch.arange(S).view(-1, 1), torch.arange(S).view(1, -1)
    seen = j <= (i + shift).clamp(0, S - 1)
    if pad_last and S > 1:
        seen = seen & (j < S - 1)
    sc = sc.masked_fill(~seen, float("-inf"))
    lse = torch.logsumexp(sc, -1)
    p = torch.exp(sc - lse[..., None])
    o = (p @ vv).permute(0, 2, 1, 3).reshape(B * S, Hq * 64)
    return o, lse, p[:, :, S - 1], p.sum(-2)


def score_eps(q, k, S):
    """eps_s = 2^-21 A, A = max over the unmasked (i, j) of sum_d |q_id k_jd|: the score error of 22-bit operand
    planes (two fp16 planes at a power-of-two scale, or three bf16 planes, keep at least 22 bits of every element)."""
    G = q.shape[1] // k.shape[1]
    a = q.double().abs() @ k.double().abs().repeat_interleave(G, 1).transpose(-1, -2)
    return float(torch.tril(a).max()) * 2.0 ** -21


def edge_caps(q, k, v, o_ref, S):
    """The derived caps of the fp32 kernels' errors against fp64 (and of the CPU fp32 oracle's, the yardstick): a
    score is off by at most eps_s, a probability then by about 2 eps_s relative; the floors are those of
    test_attention_f32 / test_importance_stats_f32 at the old shapes.  o, lastrow, colsum: max |err| / max |ref|;
    lse: max |err|."""
    e = score_eps(q, k, S)
    return {"o": 1e-5 + 4 * e * float(v.abs().max()) / max(float(o_ref.abs().max()), 1e-30),
            "lse": 5e-5 + 2 * e, "lastrow": 2e-6 + 4 * e, "colsum": 5e-6 + 4 * e}


def edge_err(name, got, ref):
    """The error measure of ``edge_caps``; a non-finite output is an infinite error."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    if not torch.isfinite(got).all():
        return float("inf")
    d = float((got - ref).abs().max())
    return d if name == "lse" else d / max(float(ref.abs().max()), 1e-30)


# ---- AttnLRP attention backward on ragged windows and hard rows (test_lrp_edges*.py) -------------------------------
# EDGE_S and one off the 32-row tile both backward sweeps stage (the bf16 dK/dV sweep starts at (kb * 64) & ~31)
LRP_EDGE_S = sorted(set(EDGE_S) | {31, 32, 33})
# ... and Qwen2's layout: G = 7 q heads per kv head, so with an odd tile count the group-sum sweep (one workgroup
# walks the G heads through the same two buffers) crosses a head boundary on either buffer parity
LRP_LAYOUTS = EDGE_LAYOUTS + [EDGE_LAYOUT_G16, (2, 14, 2)]
LRP_DO_KINDS = ["rand", "last", "zero_head"]
LRP_OUTPUTS = ("D", "rel", "dq", "dk", "dv")
# The row magnitudes are floored at this fraction of the output's largest row magnitude.  Under sink150 / down40 the
# column mass of most keys is ~e^-150: those rows of dk and dv are 0 in any fp32 arithmetic (exp underflows at
# e^-103) and ~1e-65 in fp64, a relative error of 1 that says nothing.  The fraction is what the number formats of
# the fp32 sweeps resolve (csrc/lrp_f32.hip; the bf16 sweeps keep fp32's exponent range on P and dS):
#   D, dv  P is held on two fp16 planes at the scale 2^14, an absolute step of 2^-39 next to the largest P = 1: a
#          row 2^-20 below the largest still has 19 bits, finer than every cap.
#   dq, dk go through dS, split at the fixed scale sd = so sv 2^-21 that rests on the bound |dS| <= 64 max|dO| max|v|.
#          With so max|dO| > 2^14 and sv max|v| > 2^14 the planes' absolute step is 2^-25 / sd < 2^-32 max|dO| max|v|,
#          while the largest a_dS (row 0: sum_d |dO_0d| |v_0d|, ~41 for the Gaussian dO and v here) is only ~3 max|dO|
#          max|v|: the bound is loose by 2^4..2^5, and a row summing n such roundings carries about sqrt(n / 12)
#          2^-33 / 3 of the largest row magnitude, 2^-32 at n = 257.  A floor of 2^-12 keeps that share of a floored
#          row at 2^-20 (1e-6), below every yardstick; at 2^-20 it alone would take 2^-12 = 2.4e-4, more than the
#          caps (the first MI355X run, with 2^-20 throughout, showed exactly that: dk up to 2.1e-4 on rows 1e-7 of
#          the largest, whose hi plane is an fp16 subnormal, and everything else as the yardstick).
LRP_FLOOR_FRAC = {"D": 2.0 ** -20, "rel": 2.0 ** -20, "dv": 2.0 ** -20, "dq": 2.0 ** -12, "dk": 2.0 ** -12}


# The CPU yardsticks' worst error (``lrp_err`` against fp64) per kind, over every length of LRP_EDGE_S, every layout of
# LRP_LAYOUTS and every dO kind, rounded up to two digits (test_lrp_edges.py ``yard_f32`` - ops.lrp_attn_bwd on CPU
# fp32 tensors after the CPU fp32 forward - and ``yard_bf16``, the bf16 sweeps' rounding points emulated on the CPU).
# flat: the scores are exact (q = 0) and dk is identically 0; sink150: key 0 has probability exactly 1.0 in fp32 and
# bf16 alike, what is left is the fp32 summation.
LRP_YARD_WORST = {
    "f32": {
        "rand": {"D": 3.6e-06, "rel": 2.0e-06, "dq": 7.7e-07, "dk": 5.1e-06, "dv": 1.5e-05},
        "flat": {"D": 2.9e-07, "rel": 1.9e-07, "dq": 1.1e-07, "dk": 0.0, "dv": 7.7e-07},
        "sink30": {"D": 3.7e-06, "rel": 1.6e-06, "dq": 3.5e-06, "dk": 4.8e-06, "dv": 2.8e-05},
        "sink150": {"D": 9.5e-08, "rel": 6.9e-08, "dq": 1.6e-07, "dk": 7.3e-08, "dv": 3.0e-07},
        "diag60": {"D": 3.3e-06, "rel": 9.1e-07, "dq": 9.7e-07, "dk": 2.8e-06, "dv": 1.5e-05},
        "ramp7.5": {"D": 6.1e-06, "rel": 2.4e-06, "dq": 7.1e-07, "dk": 5.8e-06, "dv": 2.6e-05},
        "ramp8": {"D": 6.0e-06, "rel": 4.0e-06, "dq": 7.3e-07, "dk": 5.9e-06, "dv": 2.6e-05},
        "ramp8.5": {"D": 5.3e-06, "rel": 3.3e-06, "dq": 6.8e-07, "dk": 5.8e-06, "dv": 2.8e-05},
        "ramp16": {"D": 7.7e-06, "rel": 2.4e-06, "dq": 1.3e-06, "dk": 9.2e-06, "dv": 3.8e-05},
        "down40": {"D": 3.0e-06, "rel": 1.1e-06, "dq": 7.2e-07, "dk": 2.4e-06, "dv": 1.5e-05},
    },
    "bf16": {
        "rand": {"D": 1.4e-03, "rel": 1.1e-03, "dq": 8.6e-04, "dk": 1.8e-03, "dv": 3.9e-03},
        "flat": {"D": 1.4e-03, "rel": 1.1e-03, "dq": 9.0e-04, "dk": 0.0, "dv": 3.9e-03},
        "sink30": {"D": 1.6e-03, "rel": 9.9e-04, "dq": 1.2e-03, "dk": 1.7e-03, "dv": 3.9e-03},
        "sink150": {"D": 7.9e-08, "rel": 4.5e-08, "dq": 6.1e-08, "dk": 4.7e-08, "dv": 1.7e-08},
        "diag60": {"D": 1.5e-03, "rel": 1.2e-03, "dq": 7.3e-04, "dk": 1.4e-03, "dv": 3.9e-03},
        "ramp7.5": {"D": 1.5e-03, "rel": 1.1e-03, "dq": 8.8e-04, "dk": 1.7e-03, "dv": 3.9e-03},
        "ramp8": {"D": 1.6e-03, "rel": 1.1e-03, "dq": 8.8e-04, "dk": 1.6e-03, "dv": 3.9e-03},
        "ramp8.5": {"D": 1.6e-03, "rel": 1.1e-03, "dq": 8.8e-04, "dk": 1.6e-03, "dv": 3.9e-03},
        "ramp16": {"D": 1.5e-03, "rel": 1.3e-03, "dq": 8.8e-04, "dk": 1.7e-03, "dv": 3.9e-03},
        "down40": {"D": 1.5e-03, "rel": 9.4e-04, "dq": 8.8e-04, "dk": 1.6e-03, "dv": 3.9e-03},
    },
}


def lrp_caps(yard, kid, q, k, S):
    """The caps of the sweeps' errors (``lrp_err``) against fp64: four times the worst error of the CPU yardstick of
    that precision over every case of the kind (``LRP_YARD_WORST``; the factor test_f32_gpu.py grants over the CPU fp32
    GEMM), plus, for the fp32 sweeps, 4 eps_s: their scores come from 22-bit planes, so a probability is off by about
    2 eps_s relative (``edge_caps``), twice that with the LSE of a forward on the same planes, and every output is
    linear in P.  The bf16 sweeps' scores are exact products of the rounded inputs; their caps never exceed the 2e-2
    test_lrp_gpu.py grants."""
    if yard == "bf16":
        return {n: min(4 * LRP_YARD_WORST[yard][kid][n], 2e-2) for n in LRP_OUTPUTS}
    e = score_eps(q, k, S)
    return {n: 4 * LRP_YARD_WORST[yard][kid][n] + 4 * e for n in LRP_OUTPUTS}


def lrp_dO(dkind, B, Hq, Hkv, S):
    """The upstream gradient dO [B * S, Hq * 64] (fp32):

    rand       Gaussian.
    last       Gaussian on row S - 1 of every window, exactly 0 elsewhere: the gradient of the engine's seed.
    zero_head  rand with q head 1 zeroed in every window and every q head of kv group 0 zeroed in window 0 (a head /
               a whole group whose max |dO| is 0: the ``mx == 0`` branch of the power-of-two dO scale)."""
    g = torch.Generator().manual_seed(edge_seed(B, Hq, Hkv, S) + 50000)
    dO = torch.randn(B, S, Hq, 64, generator=g)
    if dkind == "last":
        dO[:, :S - 1] = 0.0
    elif dkind == "zero_head":
        if Hq > 1:
            dO[:, :, 1] = 0.0
        dO[0, :, :Hq // Hkv] = 0.0
    elif dkind != "rand":
        raise ValueError(dkind)
    return dO.reshape(B * S, Hq * 64).contiguous()


def lrp_all64(q, k, v, dO, S, shift=0, pad_last=False):
    """fp64 AttnLRP attention backward from one explicit probability matrix, with the mask as a parameter (as
    ``attention_all64``: o and LSE are computed under the same mask).  Returns (ref, mag):

    ref  D [B, Hq, S], rel [B, Hq], dq, dk, dv [B, Hq, S, 64] by the formulas of ``ops.reference.lrp_attn_bwd``,
         dk_sum, dv_sum [B, Hkv, S, 64] (the GQA group sums), o [B * S, Hq * 64] and lse [B, Hq, S].
    mag  per output and row the cancellation-free magnitude - the same expression with every factor replaced by
         its absolute value, aD = 1/2 sum |o| |dO|, a_dS = P (1/2 |dO| |v|^T + aD), 1/2 a_dS |k|, 1/2 a_dS^T |q|,
         1/2 P^T |dO| - as the maximum over the row's 64 channels; rel: sum_i aD.  At S = 1, dq and dk are exactly
         0 in exact arithmetic (dS_00 = P (dA - D) = 0), so an error relative to |ref| would mean nothing."""
    B, Hq = q.shape[:2]
    Hkv = k.shape[1]
    G = Hq // Hkv
    qd, kk, vv = q.double(), k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    sc = qd @ kk.transpose(-1, -2)
    i, j = torch.arange(S).view(-1, 1), torch.arange(S).view(1, -1)
    seen = j <= (i + shift).clamp(0, S - 1)
    if pad_last and S > 1:
        seen = seen & (j < S - 1)
    sc = sc.masked_fill(~seen, float("-inf"))
    lse = torch.logsumexp(sc, -1)
    p = torch.exp(sc - lse[..., None])
    o = p @ vv
    dOh = dO.double().view(B, S, Hq, 64).permute(0, 2, 1, 3)
    D = 0.5 * (o * dOh).sum(-1)
    dS = p * (0.5 * dOh @ vv.transpose(-1, -2) - D[..., None])
    ref = {"D": D, "rel": D.sum(-1), "dq": 0.5 * dS @ kk, "dk": 0.5 * dS.transpose(-1, -2) @ qd,
           "dv": 0.5 * p.transpose(-1, -2) @ dOh}
    aD = 0.5 * (o.abs() * dOh.abs()).sum(-1)
    a_dS = p * (0.5 * dOh.abs() @ vv.abs().transpose(-1, -2) + aD[..., None])
    el = {"dq": 0.5 * a_dS @ kk.abs(), "dk": 0.5 * a_dS.transpose(-1, -2) @ qd.abs(),
          "dv": 0.5 * p.transpose(-1, -2) @ dOh.abs()}
    mag = {"D": aD, "rel": aD.sum(-1)}
    for n in ("dq", "dk", "dv"):
        mag[n] = el[n].amax(-1)
    for n in ("dk", "dv"):
        ref[n + "_sum"] = ref[n].view(B, Hkv, G, S, 64).sum(2)
        mag[n + "_sum"] = el[n].view(B, Hkv, G, S, 64).sum(2).amax(-1)
    ref["o"], ref["lse"] = o.permute(0, 2, 1, 3).reshape(B * S, Hq * 64), lse
    return ref, mag


def lrp_err(name, got, ref, mag):
    """max over rows (window, head, token) of max_d |got - ref| / the row's magnitude, the magnitude floored at
    ``LRP_FLOOR_FRAC`` (by output; dk_sum / dv_sum as dk / dv) of the output's largest.  A row of magnitude 0 (dk
    under q = 0, every output of a head whose dO is 0) must be exactly 0, and the output finite: otherwise the error
    is infinite."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    if not torch.isfinite(got).all():
        return float("inf")
    diff = (got - ref).abs()
    if diff.dim() > mag.dim():
        diff = diff.amax(-1)
    zero = mag == 0
    if bool((diff[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    frac = LRP_FLOOR_FRAC[name.replace("_sum", "")]
    return float((diff / mag.clamp_min(frac * float(mag.max())))[~zero].max())


# ---- GEMM family and LM-head NLL on ragged shapes and hard rows (test_gemm_edges*.py) -------------------------------
# one off the 16-row MFMA group, the 64-row wave slab, the 128-row block and the 256-row four-wave tile
GEMM_EDGE_M = [1, 2, 15, 16, 17, 63, 65, 127, 128, 129, 255, 256, 257]
GEMM_KINDS = ["rand", "outlier", "rowmag", "cancel", "onehot", "zero_rows"]
NLL_KINDS = ["rand", "peak12", "peak60", "far60", "flat", "shift200", "tie"]
NLL_EDGE_R = [1, 17, 129, 257]
U24 = 2.0 ** -24          # the unit of the GEMM measures: errors are reported in units of 2^-24 S
GELU_LIP, SILU_LIP = 1.13, 1.1   # max |gelu'| = 1.129, max |silu'| = 1.0998


def gemm_case(kind, M, N, K, seed):
    """fp32 (x [M, K], w [N, K]), seeded:

    rand       Gaussian x, Gaussian w / sqrt(K).
    outlier    rand with x[:, 3] *= 1024 and x[:, K - 1] *= 256: massive channels in the first and the last 8-element
               chunk of a K-tile row (the h3 scale is taken from them: every other channel sits 2^-8..2^-10 below it).
    rowmag     rand with row m scaled by 2^-(m % 21): rows 2^-20 below the scale's maximum.
    cancel     x[:, 1::2] = -x[:, 0::2] and w[:, 1::2] = w[:, 0::2] (1 + 2^-12 u), u uniform in [-1, 1]: every
               output is the small difference of large products, |ref| <= 2^-8 sum_k |x| |w| (test_gemm_edges.py).
    onehot     x[m, m % K] = 1 + m % 7, every other element 0; w rounded to bf16 (exact in fp16 after the power-of-two
               scale): every output is one weight entry times a small integer, exact in fp32 and in the h3 products.
    zero_rows  rand with rows 0, M // 2 and M - 1 all zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if kind in ("rand",):
        pass
    elif kind == "outlier":
        x[:, 3] *= 1024.0
        x[:, K - 1] *= 256.0
    elif kind == "rowmag":
        x *= (2.0 ** -(torch.arange(M) % 21).float()).view(-1, 1)
    elif kind == "cancel":
        x[:, 1::2] = -x[:, 0::2]
        u = torch.rand(N, K // 2, generator=g) * 2 - 1
        w[:, 1::2] = w[:, 0::2] * (1 + 2.0 ** -12 * u)
    elif kind == "onehot":
        x.zero_()
        m = torch.arange(M)
        x[m, m % K] = (1 + m % 7).float()
        w = w.bfloat16().float()
    elif kind == "zero_rows":
        x[[0, M // 2, M - 1]] = 0.0
    else:
        raise ValueError(kind)
    return x.contiguous(), w.contiguous()


def gemm_seed(M, N, K):
    return 9000 + 7 * M + 3 * N + K


def nll_special_targets(V):
    """Column 0 and V - 1, the first and the last column of the last slab of the last full 256-column tile, and one
    column in each 64-column slab of the partial last tile (V % 256 == 128; else of the last tile's first half)."""
    full = (V // 256) * 256
    part = full if V % 256 else V - 256
    return [0, V - 1, max(full - 64, 0), max(full - 1, 0), part + 5, part + 64 + 60, 63, 64]


def nll_targets(R, V):
    """(67 r + 5) % V; with R >= 17 rows 0..7 take ``nll_special_targets``; with R >= 129 rows 8..71 take every
    offset 0..63 of one slab (the slab in the middle of the vocabulary)."""
    t = (67 * torch.arange(R) + 5) % V
    if R >= 17:
        t[:8] = torch.tensor(nll_special_targets(V))
    if R >= 129:
        t[8:72] = 64 * ((V // 64) // 2) + torch.arange(64)
    return t.long()


def nll_case(kind, R, V, K, seed):
    """fp32 (h [R, K], w [V, K], targets [R]); logits h @ w.T ~ N(0, 1) (h Gaussian, w Gaussian / sqrt(K)), then:

    rand      unchanged.
    peak12 / peak60  w[t_r] = c h_r / |h_r|^2, c = 12 / 60: the target logit is c, the NLL about V e^-12 / 0.
    far60     the same row on column (t_r + V / 2) % V: maximum and target in different 64-column partials, NLL 54..66.
    flat      w = 0: NLL = log V.
    shift200  h[:, 0] = 20, w[:, 0] = -10: every logit near -200, the max subtraction is mandatory.
    tie       peak12, and its weight row copied to column t_r ^ 1 (same slab) and (t_r + 192) % V (another slab): the
              exact maximum three times (twice on the rows of the 64-offset block, whose slab is full).
    Rows sharing a column (R > V / 67, the explicit targets) overwrite one another in row order: the later row keeps
    its structure, the reference is computed from the weights as they are."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(R, K, generator=g)
    w = torch.randn(V, K, generator=g) / K ** 0.5
    t = nll_targets(R, V)
    if kind == "rand":
        pass
    elif kind in ("peak12", "peak60", "far60", "tie"):
        c = 60.0 if kind in ("peak60", "far60") else 12.0
        rows = c * h / h.pow(2).sum(-1, keepdim=True)
        col = (t + V // 2) % V if kind == "far60" else t
        taken = set(col.tolist())
        for r in range(R):
            w[col[r]] = rows[r]
            for c2 in ([int(col[r]) ^ 1, (int(col[r]) + 192) % V] if kind == "tie" else []):
                if c2 not in taken:              # (never over another row's target: the 64-offset block fills its slab)
                    w[c2] = rows[r]
    elif kind == "flat":
        w.zero_()
    elif kind == "shift200":
        h[:, 0] = 20.0
        w[:, 0] = -10.0
    else:
        raise ValueError(kind)
    return h.contiguous(), w.contiguous(), t


def nll_seed(R, V, K):
    return 11000 + 5 * R + V % 1000 + K


def h3_operands(x, w, two_term):
    """The h3 operands of x @ w.T at the tensors' own power-of-two scales -> (a3, w3, alpha, sx, sw).  ``two_term``:
    ``w`` must hold bf16 values (the single-plane weight); else the three-plane weight [N, 3K], whatever its lo plane."""
    from llm_inference_in_distributed_edge_networks_amd.ops import reference as R
    sx = R.h3_scale(float(x.abs().max()))
    w3, sw = R.h3_weight(w, two_term=two_term)
    assert w3.shape[1] == (1 if two_term else 3) * x.shape[1]
    return R.h3_act(x, sx), w3, 1.0 / (sx * sw), sx, sw


def h3_exact(a3, w3, alpha, rscale=None, colscale=None):
    """The h3 arithmetic check's reference: the planes are exact inputs and fp16 x fp16 products are exact in fp32, so
    the kernel computes alpha rscale colscale (A' @ B'^T) with fp32 accumulation only -> (that in fp64 [M, N], S =
    |scale factors| sum_k |a'_k| |b'_k|, the GEMM's K')."""
    from llm_inference_in_distributed_edge_networks_amd.ops import reference as R
    terms = R.h3_terms(a3, w3)
    A = R.h3_expand(a3, terms).double()
    B = (torch.cat([w3, w3], -1) if terms == 2 else w3).double()
    return scale_ref(A @ B.t(), A.abs() @ B.abs().t(), alpha, rscale, colscale) + (A.shape[1],)


def scale_ref(p, S, alpha, rscale=None, colscale=None):
    """(p, S) [M, N] times the product's scale factors alpha rscale[m] colscale[n] (S by their magnitudes)."""
    f = torch.full((p.shape[0], 1), float(alpha), dtype=torch.float64)
    if rscale is not None:
        f = f * rscale.double().view(-1, 1)
    if colscale is not None:
        f = f * colscale.double().view(1, -1)
    return p * f, S * f.abs()


def gemm_exact(x, w, rscale=None, colscale=None):
    """fp64 rscale colscale (x @ w.T) and S = |scales| sum_k |x_k| |w_k|: the fidelity reference of the h3 GEMMs and,
    on bf16-rounded inputs, the reference of the bf16 GEMM."""
    xd, wd = x.double(), w.double()
    return scale_ref(xd @ wd.t(), xd.abs() @ wd.abs().t(), 1.0, rscale, colscale)


def acc_cap_units(Kx):
    """(Kx + 2) 2^-23 S in units of 2^-24 S: the standard bound on a length-Kx fp32 sum in any order with at most one
    ulp per add (so it covers a truncating accumulator too), and two more roundings for the scale factors."""
    return 2.0 * (Kx + 2)


H3_DROPPED_UNITS = 8.0     # 2^-21 S: the dropped lo x lo products (2^-22) and the two planes' roundings (2^-23 each)


def h3_lo_floor(x, w, sx, sw):
    """The absolute floor of the lo planes [M, N] (rowmag, outlier): an element far below the scale's maximum keeps
    absolute accuracy, not relative.  lo = fp16(s x - hi) is an fp16 subnormal when |s x - hi| < 2^-14, i.e. for every
    |s x| < 2^-3; fp16's subnormal spacing is 2^-24, so a plane pair represents s x to within 2^-25 absolutely (and to
    2^-22 |s x| where lo is normal - H3_DROPPED_UNITS).  Per output: 2^-25 (sum_k |w_nk| / s_x + sum_k |x_mk| / s_w)."""
    fw = w.double().abs().sum(1).view(1, -1) / sx
    fx = x.double().abs().sum(1).view(-1, 1) / sw
    return 2.0 ** -25 * (fw + fx)


def plane_out_err(ref, so):
    """What reading a result back from h3 planes at scale ``so`` adds: 2^-22 |ref| (hi and lo roundings) + 2^-25 / so."""
    return 2.0 ** -22 * ref.abs() + 2.0 ** -25 / so


def add_epilogue(p, bias=None, resid=None, n_mul=1):
    """fp64 p + bias + resid and e_out, the fp32 roundings of the epilogue itself: ``n_mul`` for the product's scale
    factors, one per add."""
    e = n_mul * U24 * p.abs()
    y = p
    if bias is not None:
        y = y + bias.double().view(1, -1)
        e = e + U24 * y.abs()
    if resid is not None:
        y = y + resid.double()
        e = e + U24 * y.abs()
    return y, e


def gelu_act_eps(z, ref):
    """The device GELU's own error on the pre-activation z: erff to a few ulp of its range [-1, 1] - an absolute
    2^-23 on 1 + erf, times |z| / 2 - and three fp32 roundings of the result: 2^-22 (|z| + |ref|)."""
    return 2.0 ** -22 * (z.abs() + ref.abs())


def silu_act_eps(g, ref):
    """The device's fast SiLU on the gate g (v_exp_f32 and v_rcp_f32 at one ulp each, the exponent's argument g log2 e
    rounded once: a relative |g| 2^-24 on e^-g) and the products' roundings: (|g| + 6) 2^-23 |silu(g) u|."""
    return (g.abs() + 6.0) * 2.0 ** -23 * ref.abs()


def gemm_units(got, ref, S, e_out=None):
    """max over the elements of (|got - ref| - e_out) / S in units of 2^-24.  An element with S = 0 (a zero row) must
    be within e_out alone, and the output finite: otherwise the error is infinite."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    if not torch.isfinite(got).all():
        return float("inf")
    d = (got - ref).abs()
    if e_out is not None:
        d = (d - e_out).clamp_min(0.0)
    zero = S == 0
    if bool((d[zero] > 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((d[~zero] / S[~zero]).max()) / U24


def swiglu_ref(p, S):
    """SwiGLU of the interleaved gate|up product p [M, N] (fp64) with the product's magnitude S propagated through the
    activation's Lipschitz bound, delta = 1.1 |u| delta_g + |silu(g)| delta_u (first order) -> (ref [M, N/2], S_eff
    = 1.1 |u| S_g + |silu(g)| S_u, g): a product cap of c 2^-24 S becomes c 2^-24 S_eff, and the product's own
    rounding e_out goes the same way."""
    from llm_inference_in_distributed_edge_networks_amd.ops import reference as R
    g, u = R.deinterleave_gate_up(p)
    Sg, Su = R.deinterleave_gate_up(S)
    sg = torch.nn.functional.silu(g)
    return sg * u, SILU_LIP * u.abs() * Sg + sg.abs() * Su, g


def epilogue_ref(p, S, bias=None, resid=None, act=None, n_mul=1, extra=0.0):
    """The epilogue on the fp64 product p -> (ref, S_eff, e_out): act None: p + bias + resid; "gelu": gelu(p + bias);
    "swiglu_il": silu(gate) up of the interleaved columns.  ``extra``: a further absolute error of the product (the lo
    planes' floor).  A product cap of c 2^-24 S becomes c 2^-24 S_eff; e_out holds the epilogue's own fp32 roundings,
    ``extra`` and, for an activation, the device function's term - the product errors carried through the
    activation's Lipschitz bound."""
    if act is None:
        ref, e = add_epilogue(p, bias, resid, n_mul)
        return ref, S, e + extra
    if act == "gelu":
        z, e = add_epilogue(p, bias, None, n_mul)
        ref = torch.nn.functional.gelu(z)
        return ref, GELU_LIP * S, GELU_LIP * (e + extra) + gelu_act_eps(z, ref)
    if act == "swiglu_il":
        ref, S_eff, g = swiglu_ref(p, S)
        e_eff = swiglu_ref(p, n_mul * U24 * p.abs() + extra)[1]
        return ref, S_eff, e_eff + silu_act_eps(g, ref)
    raise ValueError(act)


# ---- LM head + cross entropy
NLL_EPS_FN = 2.0 ** -20    # __expf / logf: every exp2 / log2 at one ulp, the arguments' scalings rounded once -
# a relative 2^-22 on each of the two sums (the slab partials, their combination) and on the logarithm's argument


def nll_ref(h, w, t):
    """fp64 (nll [R], max logit, target logit, log s with s = sum exp(logit - max), A [R] = max_n sum_k |h||w|)."""
    hd, wd = h.double(), w.double()
    lg = hd @ wd.t()
    mx = lg.amax(-1)
    ls = torch.log(torch.exp(lg - mx[:, None]).sum(-1))
    tl = lg.gather(1, t.view(-1, 1)).squeeze(1)
    A = (hd.abs() @ wd.abs().t()).amax(-1)
    return mx + ls - tl, mx, tl, ls, A


def nll_cap(ref, delta_units):
    """2 max_n delta_logit + 4 2^-24 (|max logit| + |target logit| + |log s|) + eps_fn per row, with delta_logit =
    ``delta_units`` 2^-24 S the product cap of the path."""
    _, mx, tl, ls, A = ref
    return 2 * delta_units * U24 * A + 4 * U24 * (mx.abs() + tl.abs() + ls.abs()) + NLL_EPS_FN


def nll_err(got, ref, cap):
    """max over the rows of |got - ref| / cap (<= 1 passes) and the largest absolute error."""
    got = got.detach().double().cpu()
    if not torch.isfinite(got).all():
        return float("inf"), float("inf")
    d = (got - ref[0]).abs()
    return float((d / cap).max()), float(d.max())
