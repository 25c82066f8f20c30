"""Boundary codecs: what crosses a pipeline-stage boundary and how it is quantized.

The reference only *simulates* the device boundary with in-place fake
quantization of ``hidden_states`` after layer ``layer_of_interest``
(Q1 ``Experiments/Qwen2-0.5B/qwen_layer_wise.py:54-70``, Q5/Q6
``qwen_layer_wise.py:106-152``, Q2/Q4 ``Experiments/Pythia-70M/pythia_model.py:57-68,116-145``).
Here every boundary produces a real, self-describing byte message
(``wire.py``) that is shipped with RCCL ``send``/``recv`` between stages and
decoded on the receiving GPU; fake quantization is simply ``decode(encode(x))``.

Codecs (``CODECS``):

=====================  ==============  ==============  ===========  ==================================
name                   hi class        lo class        scales       reference
=====================  ==============  ==============  ===========  ==================================
passthrough            native dtype    --              --           no quantization (ratio 0)
ref_int4_global        native dtype    int4 [-8,7]     per window   Q1 (one global max-abs scale)
int4_token             native dtype    int4 [-7,7]     per token    Q1 with per-token scales
int8_token             int8            --              per token    BASELINE config 2 (uniform int8)
mixed_int4_int8        int8            int4            per token    BASELINE configs 3-5
mixed_int2_int8        int8            int2 ternary    per token    extra compression point
channel_8 / channel_4  int8 / int4     --              per channel  Q5
channel_1_mean/_max    int2 ternary    --              per channel  Q6
int8_token_keep        native dtype    int8            per token    Q2/Q4 (Pythia 'initial', intended semantics)
mxfp4 / mxfp8          MXFP4 / MXFP8   --              E8M0 / 32ch  OCP microscaling, every token (gfx950
                                                                    scaled converts)
mixed_mxfp4_mxfp8      MXFP8 (E4M3)    MXFP4 (E2M1)    E8M0 / 32ch  configs 3-5 at microscaling widths
mxfp4_keep             native dtype    MXFP4           E8M0 / 32ch  Q1 with MX blocks instead of one scale
(the three above)      with_mx_elem "e2m3" / "e3m2": their MXFP4    MXFP6 rows, 6.25 bits per element
                       rows as FP6 E2M3 / E3M2 codes                (gfx950 2xpk16 / pk32 fp6 converts)
(the three above)      with_mx_elem "nvfp4": their MXFP4 rows as    E2M1 codes, an E4M3 scale per 16 channels,
                       NVFP4 rows, 4.5 bits per element             one fp32 scale a row (lane pairs, one DPP move)
(the four above)       with_mx_rot "h32": their MX rows as the      the plain rows' bytes of y = H32 x / 4 per
                       rotated twins of the same element type       32-channel block (Hadamard, quad DPP moves)
(the int rows above)   with_outliers "top8": the int8 / int4 /      the row's 8 largest channels cross as exact
                       int2 rows of the per-token codecs            fp32 beside it; the scale is the rest's
(the int rows above)   with_row_rot "h128": the same rows as        the plain rows' bytes of y = H128 x / 8 per
                       their rotated twins (H % 128 == 0)           128-channel block (Hadamard, DPP row moves)
(the int rows above)   with_row_rot "full": the same rows, one      the plain rows' bytes of y = e H x, H of order
                       rotation of the row (H = 2^n, 28 x 2^m)      H: Sylvester, or Paley H28 (x) Sylvester
rgroup                 head groups     --              per group    every 64-channel group (one head) its
                                                                    own max-abs scale and 2/4/8-bit width
mixed_rgroup_int8      int8            head groups     token/group  config 5 (relevance-allocated widths
                                                                    from channel_group_relevance.json)
rgroup_rot             rotated groups  --              per group    rgroup's bytes of y = H64 x / 8 (64-point
                                                                    Walsh-Hadamard, QuaRot / SpinQuant)
=====================  ==============  ==============  ===========  ==================================

Head-group codecs carry their group bit plan in the message; a boundary's plan comes from
``plan.allocate_group_bits`` over the LRP relevance of its 64-channel groups (uniform without a table).

``rgroup_rot`` rotates every group with the orthonormal Hadamard matrix before quantizing and back after
dequantizing (integer butterflies on the codes, bit-identical on CPU and GPU), so a massive channel no longer sets
its group's step alone: reconstruction MSE on a randn input with one x100 channel per group is 2.2x (4 bits) / 48x
(8 bits) below ``rgroup``'s and unchanged on plain Gaussians.  At 3 bits it loses there (0.41x): ``rgroup`` zeroes
the small channels and its error stays bounded by their variance.  In the default plan mode its plans are allocated
from the UNROTATED sensitivity / relevance tables; ``group_plan: "measured"`` allocates them (and ``rgroup``'s) exactly
against the quantization error the relevance pass measures per group and width in the rotated (plain) basis
(``plan.allocate_group_bits_measured``, ``channel_group_quant_error.json``).

The "native dtype" rows cross as fp32 (4 B per element) in the fp32 execution mode; ``with_native_wire(spec, "bf16" |
"fp16" | "fp16s")`` (params key ``native_wire``) sends them as 16-bit rows instead - bf16, IEEE fp16 (overflows to Inf
past 65504: loud) or fp16 with a per-row power-of-two scale (no finite row overflows, 8x below bf16's rounding error);
see ``wire.py``.  BASELINE config 1 ("fp16 pass-through") is ``passthrough`` with ``"native_wire": "fp16"``.

``with_mx_elem(spec, "e2m3" | "e3m2")`` (params key ``mx_elem``) fills the MX family's gap between 4.25 (``mxfp4``) and
8.25 (``mxfp8``) bits per element: the codec's MXFP4 rows become MXFP6 rows - 32-channel E8M0 blocks of FP6 E2M3 (max
7.5) or E3M2 (max 28) codes, 25 H / 32 bytes a row.  A modifier like ``with_native_wire``, not a new codec; not combined
with a 16-bit native wire.  ``with_mx_elem(spec, "nvfp4")`` sends the same rows as NVFP4 rows instead: E2M1 codes in
blocks of 16 channels with an E4M3 scale each and one fp32 scale a row, 9 H / 16 + 4 bytes - the point between ``fp4``
and ``e2m3``; not combined with ``with_mx_rot`` either.

``with_mx_rot(spec, "h32")`` (params key ``mx_rot``) puts a 32-point Hadamard transform in front of every MX block's
quantizer and behind its dequantizer, at the plain row's bytes: one loud channel of a block no longer sets the scale
that flushes the block's other 31.  It composes with ``with_mx_elem`` and is the one rotation that meets importance
selection (``mixed_mxfp4_mxfp8``, ``mxfp4_keep``); not combined with a 16-bit native wire.

``with_outliers(spec, "top8")`` (params key ``outliers``) is the per-token int rows' answer to massive activations
(LLM.int8 / SpQR): the 8 channels of a row with the largest magnitude cross exactly, as 8 fp32 values and 8 uint16
channels after the row's codes (48 bytes a row), and the row's scale is the max-abs of the other H - 8 channels - one
loud channel no longer rounds the rest of an int4 / int2 row to zero.  For ``int4_token``, ``int8_token``,
``mixed_int4_int8``, ``mixed_int2_int8`` and ``int8_token_keep``; not combined with the other modifiers.

``with_row_rot(spec, "h128")`` (params key ``row_rot``) is the other remedy for the same rows and codecs (QuaRot /
SpinQuant): every 128-channel block of a per-token int row is quantized in the basis of the orthonormal 128-point
Hadamard transform, at the plain row's bytes (896 = 7 x 128; the hidden size must be a multiple of 128).  A loud
channel is spread over its block, so the row's max-abs and step fall by up to 8.  It pays where the spread spike stays
within a few steps of the other channels - int8 rows, moderate spikes at int4; at 2 bits and for very large spikes at
4 bits it can lose, and ``with_outliers`` is the remedy there.  Not combined with the other modifiers.

``with_row_rot(spec, "full")`` rotates the whole row instead, as QuaRot / SpinQuant do: one Hadamard matrix of order H,
the Sylvester matrix for H = 2^7 .. 2^12 and H28 (x) H_2^m (H28: Paley type II, q = 13) for H = 896, 1792, 3584; any
other hidden size is a ``ValueError`` (12 x 2^k and 20 x 2^k sizes are out of scope).  The row's max-abs falls by up to
sqrt(H) instead of 8: int8 rows with one x100 channel reconstruct with 3.3x less error than under ``h128``.  Where
rotation loses - int4 with a x1000 channel, int2 - it loses by more than ``h128``; ``with_outliers`` stays the remedy.

``fake_quant_fork(x, spec, B, S, variants, importances)`` is ``fake_quant`` for a whole list of (importance source, k)
variants of one codec at once - the sweep's step between the shared prefix and the stacked suffix: one sort per
source, one read of ``x``, one write per variant, bit-identical to the per-variant round trip (``fork_supported``: the
native / int8 / int4 / int2 codecs with per-token or per-window scales, ratio selection, native wire).

"hi"/"lo" classes: the ``k = int(ratio * S)`` least important tokens of a
window (ascending importance, ties broken by position) are the lo class.
"""
from . import plan  # noqa: F401  (codec.plan: the head-group bit plans)
from .wire import (CODECS, CodecSpec, Layout, decode, encode, fake_quant, fake_quant_fork, fork_supported, get_codec,
                   layout, message_bytes, select_mask, with_mx_elem, with_mx_rot, with_native_wire, with_outliers,
                   with_row_rot)

__all__ = ["CODECS", "CodecSpec", "Layout", "decode", "encode", "fake_quant", "fake_quant_fork", "fork_supported",
           "get_codec", "layout", "message_bytes", "select_mask", "with_mx_elem", "with_mx_rot",
           "with_native_wire", "with_outliers", "with_row_rot"]
