"""Wire format of a boundary message and the encode/decode entry points.

Message for a micro-batch of ``B`` windows of ``S`` tokens, hidden size ``H``,
``k`` lo-class tokens per window (all sections 16-byte aligned)::

    header   32 B   int32[8] = magic 'EDGB', version, codec id, B, S, H, k (-1: variable), hi-row format
    mask     B * MW uint32        bit j of window b set <=> token j is in the lo class (MW = 2*ceil(S/64))
    scales   fp32                 per token [B*S] | per window [B] | per channel [B*H]
    hi rows  B*(S-k) rows         token order within each window
    lo rows  B*k rows             token order within each window

The size depends only on (codec, B, S, H, k, native dtype), so sender and
receiver agree on it without a handshake and the receiver can post its
``irecv`` before the sender has produced anything.

Selection.  ``"ratio"`` (the reference): the ``k = int(ratio*S)`` least important tokens of
every window.  ``"top_rho"`` (Pythia ``'upto ratio'``, ``pythia_model.py:92-112``): each
window keeps the shortest prefix of its tokens by descending importance whose mass reaches
``1 - ratio`` and quantizes the rest, so k varies per window.  That message carries
``k`` per window after the mask and stores the lo rows first and the hi rows right after
the ``sum k`` lo rows (compact); its buffer (``Layout.total``) has capacity for any k and
``payload_bytes(sum_k)`` is what a link would carry.

16-bit wire formats.  The rows a codec keeps in the activation dtype (hi or lo format ``NATIVE``: ``passthrough``,
``ref_int4_global``, ``int4_token``, ``int8_token_keep``, ``mxfp4_keep``) cross as fp32, 4 B per element, in the fp32
execution mode.  ``with_native_wire(spec, name)`` - a modifier of a ``CodecSpec`` like ``with_plan``, not a new codec -
sends them in a 16-bit row format instead; the header's hi-row-format word then carries 0, 9 or 10:

* ``"bf16"``  (``FMT_BF16`` = 0): round to nearest even, 2 H bytes a row; fp32's range, 8 significant bits.
* ``"fp16"``  (``FMT_F16`` = 9): IEEE binary16, round to nearest even, 2 H bytes; subnormals and -0 kept.  A finite
  value that rounds past 65504 encodes as +-Inf and decodes non-finite - loud, never clipped: for unbounded data (the
  massive activations of Qwen2-class residual streams) use ``"fp16s"`` or ``"bf16"``.
* ``"fp16s"`` (``FMT_F16S`` = 10): scaled fp16, H binary16 codes then one fp32 ``p``, 2 H + 4 bytes.  ``p = 2^k``,
  ``k = clamp(E - 141, -112, 113)`` from the biased exponent ``E`` of the row's max-abs (p = 1 for an all-zero row,
  p = the max-abs itself for a row holding a NaN / Inf, which decodes non-finite throughout); code =
  ``fp16(x * 2^-k)``, decode = ``float(code) * p``.  The row's largest value lands in [2^14, 2^15), so no finite row
  overflows, and ``|x' - x| <= max(2^-11 |x|, 2^(k - 25))``: 8x below bf16's rounding error.
* ``"native"``: the activation dtype, as without the modifier.

MXFP6 rows.  ``with_mx_elem(spec, name)`` - a modifier too - resolves every ``FMT_MXFP4`` class of a codec (``mxfp4``,
``mixed_mxfp4_mxfp8``'s lo rows, ``mxfp4_keep``'s lo rows) to an OCP MX 6-bit element type at 6.25 bits per element,
between mxfp4's 4.25 and mxfp8's 8.25:

* ``"e2m3"`` (``FMT_MXFP6`` = 11): FP6 E2M3, bias 1, largest value 7.5, emax 2.
* ``"e3m2"`` (``FMT_MXBF6`` = 12): FP6 E3M2, bias 3, largest value 28, emax 4.
* ``"fp4"``: E2M1, as without the modifier.

Neither 6-bit type has Inf / NaN codes, both have subnormals.  Row = ``[codes][H/32 E8M0 bytes]`` as for every MX row; a
block's 32 six-bit codes are one little-endian bit stream of 24 bytes, code c at bits [6c, 6c + 6), sign in the code's
top bit: 25 H / 32 bytes a row.  Code = round to nearest even of ``clamp(x / X, +-max)`` on the element grid (X the
block's E8M0 scale; the clamp first: x / X reaches (7.5, 8) and (28, 32)).  With the modifier on, header word 7 is
``hi_fmt | lo_fmt << 8``, and ``decode`` refuses a message whose formats are not its spec's.  Not combined with a 16-bit
native wire, and such specs are not served by ``fake_quant_fork``.

Rotated MX rows.  ``with_mx_rot(spec, "h32")`` - a modifier too - resolves every MX class of a codec (the rows of
``mxfp4``, ``mxfp8`` and ``mixed_mxfp4_mxfp8``, the lo rows of ``mxfp4_keep``; after ``with_mx_elem``) to its rotated twin
(``FMT_MXFP4R`` = 13, ``FMT_MXFP8R`` = 14, ``FMT_MXFP6R`` = 15, ``FMT_MXBF6R`` = 16): the plain row's bytes, but codes
and scale byte describe ``y = H32 x / 4`` of every 32-channel block, H32 the natural-order Sylvester matrix
(``y_i = sum_j (-1)^popcount(i & j) x_j``) - one loud channel of a block is spread over all 32, so the block's scale no
longer flushes its small channels.  Encode: five fp32 butterfly stages ``(a, b) -> (a + b, a - b)`` at channel strides
1, 2, 4, 8, 16 (the lower index keeps the sum), one multiply by 0.25, then the plain row's quantizer.  Decode: the
plain row's values, the same five stages, one multiply by 0.125 (H32 H32 = 32 I).  The decoder's sums are multiples of
the grid quantum below 2^24 of them, so exact.  A block holding a NaN / Inf, or a finite one whose butterflies overflow
(max-abs from about 2^123 up), stores byte 255 and decodes to 32 NaNs.  Header word 7 is ``hi_fmt | lo_fmt << 8``.  Not
combined with a 16-bit native wire; such specs are not served by ``fake_quant_fork``.

Outlier rows.  ``with_outliers(spec, "top8")`` - a modifier too - resolves every ``FMT_INT8`` / ``FMT_INT4`` /
``FMT_INT2`` class of a per-token codec (``int4_token``, ``int8_token``, ``mixed_int4_int8``, ``mixed_int2_int8``,
``int8_token_keep``) to its outlier twin (``FMT_INT8O`` = 17, ``FMT_INT4O`` = 18, ``FMT_INT2O`` = 19), the LLM.int8 /
SpQR remedy for massive activations: a row's one scale is ``max|x| / qmax``, so one loud channel rounds the other
H - 1 to zero at 4 or 2 bits.  Row = ``[the plain twin's code bytes][8 fp32 values][8 uint16 channels]``, the twin's
bytes + 48 (the code sections are multiples of 8 bytes, the tail is 4-byte aligned); the per-token scale stays in the
message's scale section.  On both sides:

1. the 8 outliers are the channels with the largest ``abs_bits(x)`` - the unsigned bit pattern of ``|x|``, the order of
   the codec's max-abs: NaN > Inf > finite - ties going to the lower channel, listed in that order;
2. a stored value is the activation's exact bits as fp32 (-0 stays -0);
3. the 8 channels are replaced by +0, the scale is ``max|rest| / qmax`` and the codes are the plain twin's of the rest;
4. decode is the plain twin's, then pair 0 .. 7 overwrites its channel.

So an all-zero row lists channels 0 .. 7 with value 0; up to 8 non-finite values cross exactly and the rest of the row
stays finite; from the 9th on the rest's scale is non-finite and the rest decodes non-finite - loud, not clipped; a
channel >= H in a received row decodes that whole row to NaN.  The count is fixed by the format (8), not an argument.
Header word 7 is ``hi_fmt | lo_fmt << 8``.  Not for per-window / per-channel scales (``ref_int4_global`` stays the
reference's Q1 bit for bit), not for codecs with head-group rows, not combined with a 16-bit native wire, ``mx_elem``
or ``mx_rot``; such specs are not served by ``fake_quant_fork``.

Rotated per-token int rows.  ``with_row_rot(spec, "h128")`` - a modifier too - resolves every ``FMT_INT8`` / ``FMT_INT4``
/ ``FMT_INT2`` class of the same per-token codecs to its rotated twin (``FMT_INT8R`` = 20, ``FMT_INT4R`` = 21,
``FMT_INT2R`` = 22), the QuaRot / SpinQuant remedy for the same massive channels: the plain row's bytes (its codes; the
per-token scale in the message's scale section), but codes and scale describe ``y = H128 x / 8`` of every 128-channel
block, H128 the natural-order Sylvester matrix as H32 above - block-diagonal, so it needs ``H % 128 == 0`` (896 = 7 x
128; ``layout`` raises otherwise), and a loud channel is spread over its block: the row's max-abs, and with it its one
step, falls by up to 8.  Encode: seven fp32 butterfly stages ``(a, b) -> (a + b, a - b)`` at channel strides 1, 2, 4, 8,
16, 32, 64 (the lower index keeps the sum), one multiply by 0.125, then the plain row's quantizer.  Decode: the integer
codes as floats, the same seven stages (sums at most 128 x 127: exact), one multiply by ``s * 0.0625`` (H128 H128 = 128
I).  No add follows a multiply on either side, so the GPU's message is the CPU's byte for byte.  The unit is the token
row: a NaN / Inf in any block makes that block's y, hence the row's scale, hence the whole decoded row non-finite.
Overflow of the rotation: so does a finite row whose butterflies overflow (max-abs from about 2^120 up) - loud, never
clipped.  Header word 7 is ``hi_fmt | lo_fmt << 8``.  Rotation pays where the spread spike stays within a few steps of
the other channels (int8; moderate spikes at int4); at 2 bits and for very large spikes at 4 bits it can lose, and
``with_outliers`` is the remedy.  Not combined with ``native_wire``, ``mx_elem``, ``mx_rot`` or ``outliers``; such
specs are not served by ``fake_quant_fork``.

Row-rotated per-token int rows.  ``with_row_rot(spec, "full")`` - the same option's other value - resolves the same
classes to ``FMT_INT8F`` = 23, ``FMT_INT4F`` = 24, ``FMT_INT2F`` = 25: the plain row's bytes again, but codes and scale
describe ``y = e H x`` of the whole row, as QuaRot / SpinQuant rotate the whole hidden dimension - a loud channel is
spread over all H channels and the row's max-abs falls by up to sqrt(H), not sqrt(128).  Supported hidden sizes
(``ROW_ROT_FULL_SIZES``; ``layout`` raises a ``ValueError`` naming them for any other, 384 and 640 included; 12 x 2^k and
20 x 2^k sizes such as 1536 are out of scope): ``H = 2^n``, n = 7 .. 12 - H the natural-order Sylvester matrix, stages at
strides 1 .. 2^(n-1), ``e = 2^-floor(n/2)``, decode factor ``s 2^-ceil(n/2)``, so at H = 128 the message is the ``h128``
message apart from the format words; and ``H = 28 x 2^m``, m = 5, 6, 7 (896, 1792, 3584) - channel ``a 2^m + b``,
``H = H28 (x) H_2^m`` with H28 the Paley type II matrix for q = 13 (``_h28``: from the formula, symmetric, +-1,
``H28 H28 = 28 I``).  Encode: the m Sylvester stages along b; the 28-point stage ``out[a'] = sum_a H28[a'][a] t[a]``
accumulated in fp32 in ascending a from ``+-t[0]`` (the order is part of the format: it makes non-integer rows
byte-identical on GPU and CPU); one multiply by ``e = 2^-(2 + floor(m/2))``.  Decode: the codes as floats, the same
28-point routine (sums at most 3584 x 127: exact), the m stages, one multiply by ``s d`` with ``d = fp32(1/28)
2^(2 + floor(m/2) - m)``, ``s d`` rounded once.  No add follows a multiply.  The unit is the token row: a NaN / Inf
anywhere, or a finite row whose sums overflow (max-abs from about 2^(127 - log2 H)), makes the scale and the whole
decoded row non-finite.  Header word 7, the refusals and the combinations are ``h128``'s.  It is ahead of ``h128``
wherever ``h128`` is ahead of the plain row, and further behind where rotation loses (int4 with a x1000 channel, int2):
that regime is ``with_outliers``'.

NVFP4 rows.  ``with_mx_elem(spec, "nvfp4")`` - the same option's fourth value - resolves the same ``FMT_MXFP4`` classes to
``FMT_NVFP4`` = 26: E2M1 codes in blocks of 16 channels, each with an E4M3 scale (OCP e4m3fn, bias 7, 3 mantissa bits,
subnormals kept) instead of MXFP4's power of two shared by 32, and one fp32 second-level scale ``g`` a row that keeps the
E4M3 scales in range: 4.5 bits per element plus 32 / H.  The row is self-scaled::

    [H/2 code bytes][H/16 E4M3 scale bytes][g: one fp32, little-endian]        9H/16 + 4 bytes  (H = 896: 508)

Channel 2p is the low nibble of byte p; the scale byte of block j (channels [16j, 16j + 16)) is byte ``H/2 + j``; rows
are byte-aligned only.  Encode, every step one fp32 operation rounded once, ``/`` the correctly rounded quotient:

1. ``g = am / 2688`` with ``am`` the row's max-abs (2688 = 448 x 6: the loudest block's scale is the E4M3 maximum).  A
   NaN / Inf in the row makes ``g`` non-finite.
2. per block ``w = (amb / g) / 6`` with ``amb`` the block's max-abs, and ``sb`` the E4M3 round-to-nearest-even byte of
   ``min(w, 448)`` (the clamp first: the convert does not saturate; a NaN ``w`` takes 448 too, so the bytes 0x7F / 0xFF
   are never written).  ``g == 0`` (an all-zero row): every ``sb`` and code is 0.
3. ``d = e4m3(sb) * g``.  ``sb == 0`` or ``d < 2^-126``: the block's codes are 0.  Otherwise code = E2M1 round to nearest,
   ties to the even code, of ``clamp(x / d, +-6)``, the sign kept on values that round to zero.

Decode: ``d`` as in step 3 from the stored bytes, value = ``e2m1(code) * d``.  No add follows a multiply.  The unit of
the non-finite rule is the token row: a row whose ``g`` is non-finite decodes to NaN throughout, and only its code and
scale bytes may differ between GPU and CPU; a received scale byte 0x7F / 0xFF decodes its 16 channels to NaN.  Rows with
a max-abs near 2^-126 and below fall under ``d < 2^-126`` and decode to +0: finite and bounded, not accurate.  Header
word 7 is ``hi_fmt | lo_fmt << 8`` and ``decode`` refuses a message whose formats are not its spec's.  Not combined with
``native_wire`` 16-bit rows, ``mx_rot`` (rotation of 16-channel blocks is out of scope), ``outliers`` or ``row_rot``; such
specs are not served by ``fake_quant_fork``.

``encode``/``decode`` run the gfx950 kernels of ``csrc/codec.hip`` for CUDA
tensors and a bit-identical PyTorch implementation for CPU tensors.

Non-finite activations stay loud: a unit (token row, head group, MX block, window, channel) that holds a NaN or an
Inf decodes to non-finite values - its max-abs, and with it its scale, is non-finite on both sides; an MX block
stores E8M0 byte 255.  Only the bytes of such a unit may differ between the GPU and the CPU (NaN payloads).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Callable

import torch

from ..ops._native import call, ptr, stream

MAGIC = 0x45444742
VERSION = 1
FMT_BF16, FMT_INT8, FMT_INT4, FMT_INT2, FMT_F32, FMT_MXFP4, FMT_MXFP8, FMT_GRP = 0, 1, 2, 3, 4, 5, 6, 7
FMT_GRPR = 8                # FMT_GRP bytes whose codes and scales describe the Hadamard-rotated group
FMT_F16, FMT_F16S = 9, 10   # 16-bit wires of NATIVE rows: IEEE binary16; binary16 codes + one fp32 power-of-two scale
FMT_MXFP6, FMT_MXBF6 = 11, 12   # MX rows of FP6 E2M3 / E3M2 codes (with_mx_elem)
MX6_FORMATS = (FMT_MXFP6, FMT_MXBF6)
MX_FORMATS = (FMT_MXFP4, FMT_MXFP8) + MX6_FORMATS
FMT_MXFP4R, FMT_MXFP8R, FMT_MXFP6R, FMT_MXBF6R = 13, 14, 15, 16   # MX rows of the Hadamard-rotated blocks (with_mx_rot)
MX_ROT_TWIN = {FMT_MXFP4: FMT_MXFP4R, FMT_MXFP8: FMT_MXFP8R, FMT_MXFP6: FMT_MXFP6R, FMT_MXBF6: FMT_MXBF6R}
FMT_INT8O, FMT_INT4O, FMT_INT2O = 17, 18, 19   # per-token int rows + the row's 8 largest channels exact (with_outliers)
OUT_TWIN = {FMT_INT8: FMT_INT8O, FMT_INT4: FMT_INT4O, FMT_INT2: FMT_INT2O}
OUT_K, OUT_TAIL = 8, 48     # outliers of such a row; bytes of its tail: 8 fp32 values, 8 uint16 channels
FMT_INT8R, FMT_INT4R, FMT_INT2R = 20, 21, 22   # per-token int rows of the Hadamard-rotated 128-channel blocks (with_row_rot)
ROW_ROT_TWIN = {FMT_INT8: FMT_INT8R, FMT_INT4: FMT_INT4R, FMT_INT2: FMT_INT2R}
FMT_INT8F, FMT_INT4F, FMT_INT2F = 23, 24, 25   # per-token int rows of the Hadamard-rotated whole row (with_row_rot "full")
ROW_ROT_FULL_TWIN = {FMT_INT8: FMT_INT8F, FMT_INT4: FMT_INT4F, FMT_INT2: FMT_INT2F}
FMT_NVFP4 = 26              # E2M1 codes in 16-channel blocks with E4M3 scales and one fp32 scale a row (with_mx_elem "nvfp4")
NV_FORMATS = (FMT_NVFP4,)   # not in MX_FORMATS: those rows have E8M0 scale bytes
ROW_ROT_FULL = -1           # CodecSpec.row_rot of "full": the block is the row
ROW_ROT_FULL_SIZES = tuple(1 << n for n in range(7, 13)) + tuple(28 << m for m in (5, 6, 7))   # 2^n; 28 * 2^m
GRP_FORMATS = (FMT_GRP, FMT_GRPR)
SC_TOKEN, SC_WINDOW, SC_CHANNEL, SC_NONE = 0, 1, 2, 3
CH_MAXABS, CH_MEAN = 0, 1
NATIVE = -1  # "keep in the activation dtype" (bf16 on GPU, fp32 in the CPU reference mode)
NATIVE_WIRES = {"native": NATIVE, "bf16": FMT_BF16, "fp16": FMT_F16, "fp16s": FMT_F16S}   # with_native_wire
MX_ELEMS = {"fp4": FMT_MXFP4, "e2m3": FMT_MXFP6, "e3m2": FMT_MXBF6, "nvfp4": FMT_NVFP4}     # with_mx_elem
MX_ROTS = {"none": 0, "h32": 32}                                                            # with_mx_rot: block size
OUTLIERS = {"none": 0, "top8": OUT_K}                                                       # with_outliers: count
ROW_ROTS = {"none": 0, "h128": 128, "full": ROW_ROT_FULL}                                   # with_row_rot: block size


@dataclass(frozen=True)
class CodecSpec:
    name: str
    cid: int
    hi_fmt: int
    lo_fmt: int
    scale_mode: int
    qmax_hi: int = 0
    qmax_lo: int = 0
    ch_kind: int = CH_MAXABS
    uses_ratio: bool = True      # lo class = int(ratio*S) least important tokens
    needs_importance: bool = True
    plan: tuple | None = None    # FMT_GRP / FMT_GRPR rows: bits (GROUP_BITS) of every 64-channel group (with_plan)
    native_wire: int = NATIVE    # row format of the NATIVE classes on the wire (with_native_wire); NATIVE: the dtype's
    mx_elem: int = FMT_MXFP4     # row format of the FMT_MXFP4 classes on the wire (with_mx_elem)
    mx_rot: int = 0              # 32: the MX classes cross as their rotated twins (with_mx_rot); 0: as they are
    outliers: int = 0            # 8: the per-token int classes cross as their outlier twins (with_outliers); 0: as they are
    row_rot: int = 0             # 128 / ROW_ROT_FULL: the per-token int classes cross as their block- / row-rotated twins
                                 # (with_row_rot); 0: as they are


CODECS = {c.name: c for c in [
    CodecSpec("passthrough", 0, NATIVE, NATIVE, SC_NONE, uses_ratio=False, needs_importance=False),
    CodecSpec("ref_int4_global", 1, NATIVE, FMT_INT4, SC_WINDOW, 0, 7),
    CodecSpec("int4_token", 2, NATIVE, FMT_INT4, SC_TOKEN, 0, 7),
    CodecSpec("int8_token", 3, FMT_INT8, FMT_INT8, SC_TOKEN, 127, 127, uses_ratio=False, needs_importance=False),
    CodecSpec("mixed_int4_int8", 4, FMT_INT8, FMT_INT4, SC_TOKEN, 127, 7),
    CodecSpec("mixed_int2_int8", 5, FMT_INT8, FMT_INT2, SC_TOKEN, 127, 1),
    CodecSpec("channel_8", 6, FMT_INT8, FMT_INT8, SC_CHANNEL, 127, 127, CH_MAXABS, False, False),
    CodecSpec("channel_4", 7, FMT_INT4, FMT_INT4, SC_CHANNEL, 7, 7, CH_MAXABS, False, False),
    CodecSpec("channel_1_mean", 8, FMT_INT2, FMT_INT2, SC_CHANNEL, 1, 1, CH_MEAN, False, False),
    CodecSpec("channel_1_max", 9, FMT_INT2, FMT_INT2, SC_CHANNEL, 1, 1, CH_MAXABS, False, False),
    CodecSpec("int8_token_keep", 10, NATIVE, FMT_INT8, SC_TOKEN, 0, 127),
    # OCP microscaling (32-channel blocks, E8M0 scales inline in the row; gfx950 scaled converts)
    CodecSpec("mxfp4", 11, FMT_MXFP4, FMT_MXFP4, SC_NONE, uses_ratio=False, needs_importance=False),
    CodecSpec("mxfp8", 12, FMT_MXFP8, FMT_MXFP8, SC_NONE, uses_ratio=False, needs_importance=False),
    CodecSpec("mixed_mxfp4_mxfp8", 13, FMT_MXFP8, FMT_MXFP4, SC_NONE),
    CodecSpec("mxfp4_keep", 14, NATIVE, FMT_MXFP4, SC_NONE),
    # head-group rows (FMT_GRP): every 64-channel group (one head's width) has its own bit width and max-abs scale;
    # the widths come from the relevance of the boundary's channel groups (group_bits / allocate_group_bits)
    CodecSpec("rgroup", 15, FMT_GRP, FMT_GRP, SC_NONE, uses_ratio=False, needs_importance=False),
    CodecSpec("mixed_rgroup_int8", 16, FMT_INT8, FMT_GRP, SC_TOKEN, 127, 0),
    # rotated head-group rows (FMT_GRPR): rgroup's bytes, but every group is quantized in the basis of the orthonormal
    # 64-point Walsh-Hadamard transform y = H64 x / 8 (QuaRot / SpinQuant), which spreads a massive channel over its
    # group: max|y| falls by up to 8 and with it the step.  Pays from 4 bits up; at 2 - 3 bits plain rgroup's error on
    # such a group is bounded by the small channels it zeroes and rotation can lose.  The model-based plan allocator is
    # fed the UNROTATED sensitivity / relevance tables; the measured one (codec/plan.py) the error in the rotated basis.
    CodecSpec("rgroup_rot", 17, FMT_GRPR, FMT_GRPR, SC_NONE, uses_ratio=False, needs_importance=False),
]}
GROUP = 64                  # channels per group of FMT_GRP / FMT_GRPR rows
GROUP_BITS = (2, 3, 4, 5, 6, 8)


def needs_plan(spec: CodecSpec) -> bool:
    return spec.hi_fmt in GRP_FORMATS or spec.lo_fmt in GRP_FORMATS


def rotated_groups(spec: CodecSpec) -> bool:
    """The codec's head-group rows are quantized in the Hadamard basis (FMT_GRPR)."""
    return FMT_GRPR in (spec.hi_fmt, spec.lo_fmt)


def with_plan(spec: CodecSpec, plan) -> CodecSpec:
    """The codec with a group bit plan (one entry per 64-channel group, each in GROUP_BITS)."""
    from dataclasses import replace
    plan = tuple(int(b) for b in plan)
    if any(b not in GROUP_BITS for b in plan):
        raise ValueError(f"group bits must be in {GROUP_BITS}, got {plan}")
    return replace(spec, plan=plan)


def has_native_rows(spec: CodecSpec) -> bool:
    return NATIVE in (spec.hi_fmt, spec.lo_fmt)


def with_native_wire(spec: CodecSpec, name: str) -> CodecSpec:
    """The codec with its NATIVE rows sent as ``name``: "native" (the activation dtype) | "bf16" | "fp16" | "fp16s"
    (module docstring).  A codec without NATIVE rows takes "native" only."""
    from dataclasses import replace
    if name not in NATIVE_WIRES:
        raise ValueError(f"native_wire must be one of {tuple(NATIVE_WIRES)}, got {name!r}")
    if name != "native" and not has_native_rows(spec):
        raise ValueError(f"codec {spec.name} keeps no rows in the activation dtype: native_wire {name!r} has nothing "
                         "to apply to")
    if name != "native" and spec.mx_elem != FMT_MXFP4:
        raise ValueError(f"native_wire {name!r} is not combined with 6-bit MX or NVFP4 rows (mx_elem)")
    if name != "native" and spec.mx_rot:
        raise ValueError(f"native_wire {name!r} is not combined with rotated MX rows (mx_rot)")
    if name != "native" and spec.outliers:
        raise ValueError(f"native_wire {name!r} is not combined with outlier rows (outliers)")
    if name != "native" and spec.row_rot:
        raise ValueError(f"native_wire {name!r} is not combined with rotated int rows (row_rot)")
    return spec if spec.native_wire == NATIVE_WIRES[name] else replace(spec, native_wire=NATIVE_WIRES[name])


def with_mx_elem(spec: CodecSpec, name: str) -> CodecSpec:
    """The codec with its FMT_MXFP4 rows sent with element type ``name``: "fp4" (E2M1, the spec itself) | "e2m3" |
    "e3m2" (MXFP6 rows) | "nvfp4" (NVFP4 rows; module docstring).  A codec without FMT_MXFP4 rows takes "fp4" only; no
    other element type is combined with a 16-bit native wire, and "nvfp4" not with rotated MX rows."""
    from dataclasses import replace
    if name not in MX_ELEMS:
        raise ValueError(f"mx_elem must be one of {tuple(MX_ELEMS)}, got {name!r}")
    if name != "fp4":
        if FMT_MXFP4 not in (spec.hi_fmt, spec.lo_fmt):
            raise ValueError(f"codec {spec.name} has no MXFP4 rows: mx_elem {name!r} has nothing to apply to")
        if spec.native_wire != NATIVE:
            raise ValueError(f"mx_elem {name!r} is not combined with a 16-bit native wire (native_wire)")
        if spec.outliers:
            raise ValueError(f"mx_elem {name!r} is not combined with outlier rows (outliers)")
        if spec.row_rot:
            raise ValueError(f"mx_elem {name!r} is not combined with rotated int rows (row_rot)")
        if MX_ELEMS[name] in NV_FORMATS and spec.mx_rot:
            raise ValueError(f"mx_elem {name!r} is not combined with rotated MX rows (mx_rot)")
    return spec if spec.mx_elem == MX_ELEMS[name] else replace(spec, mx_elem=MX_ELEMS[name])


def has_mx_rows(spec: CodecSpec) -> bool:
    return spec.hi_fmt in MX_FORMATS or spec.lo_fmt in MX_FORMATS


def with_mx_rot(spec: CodecSpec, name: str) -> CodecSpec:
    """The codec with its MX rows quantized in the basis of the 32-point Hadamard transform of every block: "none" (the
    spec itself) | "h32" (module docstring).  Composes with ``with_mx_elem``.  A codec without MX rows takes "none"
    only; rotated MX rows are not combined with a 16-bit native wire."""
    from dataclasses import replace
    if name not in MX_ROTS:
        raise ValueError(f"mx_rot must be one of {tuple(MX_ROTS)}, got {name!r}")
    if name != "none":
        if not has_mx_rows(spec):
            raise ValueError(f"codec {spec.name} has no MX rows: mx_rot {name!r} has nothing to apply to")
        if spec.native_wire != NATIVE:
            raise ValueError(f"mx_rot {name!r} is not combined with a 16-bit native wire (native_wire)")
        if spec.outliers:
            raise ValueError(f"mx_rot {name!r} is not combined with outlier rows (outliers)")
        if spec.row_rot:
            raise ValueError(f"mx_rot {name!r} is not combined with rotated int rows (row_rot)")
        if spec.mx_elem in NV_FORMATS:
            raise ValueError(f"mx_rot {name!r} is not combined with NVFP4 rows (mx_elem nvfp4)")
    return spec if spec.mx_rot == MX_ROTS[name] else replace(spec, mx_rot=MX_ROTS[name])


def with_outliers(spec: CodecSpec, name: str) -> CodecSpec:
    """The codec with the 8 largest channels of every per-token int row kept exact beside the row: "none" (the spec
    itself) | "top8" (module docstring).  For SC_TOKEN codecs with an FMT_INT8 / FMT_INT4 / FMT_INT2 class and no
    head-group rows; not combined with a 16-bit native wire, a 6-bit MX element type or rotated MX rows."""
    from dataclasses import replace
    if name not in OUTLIERS:
        raise ValueError(f"outliers must be one of {tuple(OUTLIERS)}, got {name!r}")
    if name != "none":
        if spec.scale_mode != SC_TOKEN or not (spec.hi_fmt in OUT_TWIN or spec.lo_fmt in OUT_TWIN):
            raise ValueError(f"codec {spec.name} has no per-token int rows: outliers {name!r} has nothing to apply to")
        if needs_plan(spec):
            raise ValueError(f"outliers {name!r} is not for codecs with head-group rows ({spec.name})")
        if spec.native_wire != NATIVE or spec.mx_elem != FMT_MXFP4 or spec.mx_rot:
            raise ValueError(f"outliers {name!r} is not combined with a 16-bit native wire, mx_elem or mx_rot")
        if spec.row_rot:
            raise ValueError(f"outliers {name!r} is not combined with rotated int rows (row_rot)")
    return spec if spec.outliers == OUTLIERS[name] else replace(spec, outliers=OUTLIERS[name])


def with_row_rot(spec: CodecSpec, name: str) -> CodecSpec:
    """The codec with its per-token int rows quantized in a Hadamard basis: "none" (the spec itself) | "h128" (the
    128-point transform of every 128-channel block) | "full" (one transform of the whole row, H = 2^n or 28 * 2^m;
    module docstring).  For the specs ``with_outliers`` takes:
    SC_TOKEN codecs with an FMT_INT8 / FMT_INT4 / FMT_INT2 class and no head-group rows; not combined with a 16-bit
    native wire, a 6-bit MX element type, rotated MX rows or outlier rows."""
    from dataclasses import replace
    if name not in ROW_ROTS:
        raise ValueError(f"row_rot must be one of {tuple(ROW_ROTS)}, got {name!r}")
    if name != "none":
        if spec.scale_mode != SC_TOKEN or not (spec.hi_fmt in ROW_ROT_TWIN or spec.lo_fmt in ROW_ROT_TWIN):
            raise ValueError(f"codec {spec.name} has no per-token int rows: row_rot {name!r} has nothing to apply to")
        if needs_plan(spec):
            raise ValueError(f"row_rot {name!r} is not for codecs with head-group rows ({spec.name})")
        if spec.native_wire != NATIVE or spec.mx_elem != FMT_MXFP4 or spec.mx_rot or spec.outliers:
            raise ValueError(f"row_rot {name!r} is not combined with a 16-bit native wire, mx_elem, mx_rot or outliers")
    return spec if spec.row_rot == ROW_ROTS[name] else replace(spec, row_rot=ROW_ROTS[name])


def get_codec(name: str) -> CodecSpec:
    if name not in CODECS:
        raise KeyError(f"unknown codec {name!r}; known: {sorted(CODECS)}")
    return CODECS[name]


def _a16(n: int) -> int:
    return (n + 15) // 16 * 16


def _row_bytes(fmt: int, H: int, plan=None) -> int:
    return ROW_FORMATS[fmt].row_bytes(H, plan)


def _scale_shape(mode: int, B: int, S: int, H: int):
    """Shape of the message's fp32 scale section (None: no section)."""
    return {SC_TOKEN: (B, S), SC_WINDOW: (B,), SC_CHANNEL: (B, H), SC_NONE: None}[mode]


@dataclass(frozen=True)
class Layout:
    B: int
    S: int
    H: int
    k: int            # lo tokens per window (-1: variable, see kvar)
    mw: int
    hi_fmt: int
    lo_fmt: int
    off_mask: int
    off_scale: int
    off_hi: int       # -1 when kvar (the hi section follows the sum-k lo rows)
    off_lo: int
    total: int        # bytes of the message buffer (the capacity when kvar)
    kvar: bool = False
    off_kvec: int = -1
    plan: tuple | None = None   # FMT_GRP / FMT_GRPR group bits (also stored in the message at off_plan, one byte each)
    off_plan: int = -1

    def row_bytes(self, fmt: int) -> int:
        return _row_bytes(fmt, self.H, self.plan)

    @property
    def payload_bytes_per_token(self) -> float:
        return self.total / (self.B * self.S)

    def payload_bytes(self, k_total: int | None = None) -> int:
        """Bytes of the message proper: ``total`` for fixed k; for variable k with ``k_total`` lo rows in all."""
        if not self.kvar:
            return self.total
        return self.hi_offset(k_total) + (self.B * self.S - k_total) * self.row_bytes(self.hi_fmt)

    def hi_offset(self, k_total: int) -> int:
        return self.off_hi if not self.kvar else self.off_lo + _a16(k_total * self.row_bytes(self.lo_fmt))


def native_fmt(dtype: torch.dtype) -> int:
    if dtype == torch.bfloat16:
        return FMT_BF16
    if dtype == torch.float32:
        return FMT_F32
    raise TypeError(f"unsupported activation dtype {dtype}")


def num_lo(spec: CodecSpec, ratio: float, S: int) -> int:
    """Reference truncation: ``int(ratio * S)`` (qwen_layer_wise.py:57)."""
    if not spec.uses_ratio:
        return 0
    return max(0, min(S, int(ratio * S)))


def _resolve(fmt: int, spec: CodecSpec, native: int) -> int:
    """A class's row format on the wire: the spec's, with its modifiers (native wire, MX element type, MX rotation,
    outliers, row rotation) applied."""
    if fmt == NATIVE:
        return native
    if spec.outliers:
        return OUT_TWIN.get(fmt, fmt)
    if spec.row_rot:
        return (ROW_ROT_FULL_TWIN if spec.row_rot == ROW_ROT_FULL else ROW_ROT_TWIN).get(fmt, fmt)
    fmt = spec.mx_elem if fmt == FMT_MXFP4 else fmt
    return MX_ROT_TWIN.get(fmt, fmt) if spec.mx_rot else fmt


@lru_cache(maxsize=256)
def layout(spec: CodecSpec, B: int, S: int, H: int, k: int, dtype: torch.dtype = torch.bfloat16,
           kvar: bool = False) -> Layout:
    if H % 32:
        raise ValueError("hidden size must be a multiple of 32 for the packed formats")
    nf = native_fmt(dtype) if spec.native_wire == NATIVE else spec.native_wire
    hi, lo = _resolve(spec.hi_fmt, spec, nf), _resolve(spec.lo_fmt, spec, nf)
    if spec.row_rot == ROW_ROT_FULL:
        if H not in ROW_ROT_FULL_SIZES:
            raise ValueError(f"row-rotated int rows (row_rot full) need a hidden size in {ROW_ROT_FULL_SIZES}, got {H}")
    elif spec.row_rot and H % spec.row_rot:
        raise ValueError(f"rotated int rows need a hidden size multiple of {spec.row_rot}")
    plan = None
    if hi in GRP_FORMATS or lo in GRP_FORMATS:
        if H % GROUP:
            raise ValueError(f"head-group rows need a hidden size multiple of {GROUP}")
        plan = spec.plan if spec.plan is not None else (4,) * (H // GROUP)
        if len(plan) != H // GROUP:
            raise ValueError(f"group plan has {len(plan)} entries, hidden size {H} has {H // GROUP} groups")
    rb = lambda f: _row_bytes(f, H, plan)  # noqa: E731
    mw = 2 * ((S + 63) // 64)
    off_mask = 32
    n_scale = math.prod(_scale_shape(spec.scale_mode, B, S, H) or (0,))
    # the group plan section (one byte per group) follows the mask (and the k vector)
    plan_bytes = _a16(len(plan)) if plan is not None else 0
    if kvar:
        off_kvec = off_mask + _a16(B * mw * 4)
        off_plan = off_kvec + _a16(B * 4) if plan is not None else -1
        off_scale = off_kvec + _a16(B * 4) + plan_bytes
        off_lo = off_scale + _a16(n_scale * 4)
        total = off_lo + _a16(B * S * max(rb(hi), rb(lo))) + 16
        return Layout(B, S, H, -1, mw, hi, lo, off_mask, off_scale, -1, off_lo, total, True, off_kvec, plan, off_plan)
    off_plan = off_mask + _a16(B * mw * 4) if plan is not None else -1
    off_scale = off_mask + _a16(B * mw * 4) + plan_bytes
    off_hi = off_scale + _a16(n_scale * 4)
    off_lo = off_hi + _a16(B * (S - k) * rb(hi))
    total = off_lo + _a16(B * k * rb(lo))
    return Layout(B, S, H, k, mw, hi, lo, off_mask, off_scale, off_hi, off_lo, total, False, -1, plan, off_plan)


def message_bytes(spec: CodecSpec, B: int, S: int, H: int, ratio: float, dtype=torch.bfloat16) -> int:
    return layout(spec, B, S, H, num_lo(spec, ratio, S), dtype).total


# --------------------------------------------------------------------------------------------
# CPU (reference) implementation
def _mask_words(lo: torch.Tensor, mw: int) -> torch.Tensor:
    """bool [B, S] -> int32 [B, mw] little-endian bit words."""
    B, S = lo.shape
    bits = torch.zeros(B, mw * 32, dtype=torch.int64)
    bits[:, :S] = lo.to(torch.int64)
    w = (bits.view(B, mw, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)
    return w.to(torch.int32)


def _words_to_mask(words: torch.Tensor, S: int) -> torch.Tensor:
    w = words.to(torch.int64) & 0xFFFFFFFF
    bits = (w.unsqueeze(-1) >> torch.arange(32, dtype=torch.int64)) & 1
    return bits.reshape(words.shape[0], -1)[:, :S].bool()


def _canon(imp: torch.Tensor) -> torch.Tensor:
    v = imp.float()
    return torch.where(v == 0, torch.zeros_like(v), v)   # -0 == +0 (the kernel's key canonicalisation)


def select_mask(imp: torch.Tensor, k) -> torch.Tensor:
    """bool [B, S]: the k least important tokens (ascending, ties by position, NaN last) of each window; ``k`` an
    int or a per-window sequence."""
    B, S = imp.shape
    ks = torch.as_tensor(k, dtype=torch.int64).reshape(-1).expand(B) if not isinstance(k, int) else \
        torch.full((B,), k, dtype=torch.int64)
    order = torch.sort(_canon(imp).cpu(), dim=1, stable=True).indices
    pos = torch.arange(S).view(1, S).expand(B, S)
    lo = torch.zeros(B, S, dtype=torch.bool)
    lo.scatter_(1, order, pos < ks.view(B, 1).clamp(0, S))
    return lo.to(imp.device)


def top_rho_k(imp: torch.Tensor, mass: float) -> torch.Tensor:
    """Per-window lo count of top-rho selection: keep the shortest descending-importance prefix whose mass reaches
    ``mass`` (keep = first i with sum_{j<i} desc_j >= mass; mass <= 0 keeps nothing), quantize the rest.  [B] int64.
    Descending order = the ascending stable order reversed (as csrc/codec.hip)."""
    B, S = imp.shape
    asc = torch.sort(_canon(imp).cpu(), dim=1, stable=True).values
    desc = asc.flip(1).double()
    excl = torch.cumsum(desc, 1) - desc
    ge = excl >= mass
    keep = torch.where(ge.any(1), ge.to(torch.int64).argmax(1), torch.full((B,), S, dtype=torch.int64))
    return S - keep


def _qcodes(x: torch.Tensor, spec: CodecSpec, is_lo: bool, scale_row, ch_scale) -> torch.Tensor:
    """Quantize fp32 rows [n, H] -> int codes, exactly as csrc/codec.hip does."""
    qmax = spec.qmax_lo if is_lo else spec.qmax_hi
    if spec.scale_mode == SC_TOKEN:
        inv = torch.where(scale_row > 0, 1.0 / torch.where(scale_row > 0, scale_row, torch.ones_like(scale_row)),
                          torch.zeros_like(scale_row))
        return torch.round(x * inv[:, None]).clamp(-qmax, qmax)
    if spec.scale_mode == SC_WINDOW:
        m = scale_row  # [n] (window max broadcast per row)
        safe = torch.where(m > 0, m, torch.ones_like(m))
        t = torch.round((x / safe[:, None] * float(qmax)).clamp(-(qmax + 1), qmax))
        return torch.where(m[:, None] > 0, t, torch.zeros_like(t))
    sc = ch_scale  # [n, H]
    if spec.ch_kind == CH_MEAN or qmax == 1:
        safe = torch.where(sc != 0, sc, torch.ones_like(sc))
        t = torch.round(x / safe).clamp(-1, 1)
        return torch.where(sc != 0, t, torch.zeros_like(t))
    safe = torch.where(sc > 0, sc, torch.ones_like(sc))
    t = torch.round(x / safe * float(qmax))
    return torch.where(sc > 0, t, torch.zeros_like(t))


def _pack_rows(q: torch.Tensor, fmt: int) -> torch.Tensor:
    n, H = q.shape
    qi = q.to(torch.int64)
    if fmt == FMT_INT8:
        return (qi & 255).to(torch.uint8).reshape(-1)
    if fmt == FMT_INT4:
        p = qi.reshape(n, H // 2, 2) & 15
        return (p[..., 0] | (p[..., 1] << 4)).to(torch.uint8).reshape(-1)
    if fmt == FMT_INT2:
        p = qi.reshape(n, H // 4, 4) & 3
        return (p[..., 0] | (p[..., 1] << 2) | (p[..., 2] << 4) | (p[..., 3] << 6)).to(torch.uint8).reshape(-1)
    raise ValueError(fmt)


def _unpack_rows(b: torch.Tensor, fmt: int, n: int, H: int) -> torch.Tensor:
    u = b.to(torch.int64)
    if fmt == FMT_INT8:
        v = u.reshape(n, H)
        return torch.where(v >= 128, v - 256, v).float()
    if fmt == FMT_INT4:
        u = u.reshape(n, H // 2)
        p = torch.stack([u & 15, (u >> 4) & 15], -1).reshape(n, H)
        return torch.where(p >= 8, p - 16, p).float()
    if fmt == FMT_INT2:
        u = u.reshape(n, H // 4)
        p = torch.stack([(u >> (2 * e)) & 3 for e in range(4)], -1).reshape(n, H)
        return torch.where(p >= 2, p - 4, p).float()
    raise ValueError(fmt)


def _dequant(q: torch.Tensor, spec: CodecSpec, is_lo: bool, scale_row, ch_scale) -> torch.Tensor:
    qmax = spec.qmax_lo if is_lo else spec.qmax_hi
    if spec.scale_mode == SC_TOKEN:
        return q * scale_row[:, None]
    if spec.scale_mode == SC_WINDOW:
        return q / float(qmax) * scale_row[:, None]
    if spec.ch_kind == CH_MEAN or qmax == 1:
        return q * ch_scale
    return q * ch_scale / float(qmax)


# ---- OCP microscaling rows (csrc/codec.hip mx_pack8 / mx_unpack8) ----------------------------------------------
_FP4_GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _fp4_codes(v: torch.Tensor) -> torch.Tensor:
    """E2M1 codes of v (round to nearest, ties to even code, saturating at 6), sign in bit 3 - kept on values that
    round to zero (-0, code 8), as the gfx950 scaled convert does."""
    a = v.abs()
    # thresholds between grid points; a tie goes to the even code (0, 2, 4, 6)
    c = torch.zeros_like(a, dtype=torch.int64)
    for lo, hi_excl, code in ((0.25, True, 1), (0.75, False, 2), (1.25, True, 3), (1.75, False, 4), (2.5, True, 5),
                              (3.5, False, 6), (5.0, True, 7)):
        c = torch.where(a > lo if hi_excl else a >= lo, torch.full_like(c, code), c)
    return c | torch.signbit(v).to(torch.int64) << 3


def _minifloat_grid(ebits: int, mbits: int, bias: int) -> torch.Tensor:
    """The 2^(ebits + mbits) non-negative values of a sign / exponent / mantissa format without Inf / NaN codes, by code:
    mantissa m of exponent field 0 is the subnormal m 2^(1 - bias - mbits), of field e > 0 (2^mbits + m) 2^(e - bias -
    mbits).  All exact in fp32."""
    c = torch.arange(1 << (ebits + mbits))
    e, m = c >> mbits, c & ((1 << mbits) - 1)
    return torch.where(e == 0, m, m + (1 << mbits)).float() * torch.exp2((e.clamp(min=1) - bias - mbits).float())


@dataclass(frozen=True)
class _Fp6:
    """One FP6 element type: its grid (32 values by code), the midpoints of neighbours, the 64 values by signed code."""
    grid: torch.Tensor
    mids: torch.Tensor
    values: torch.Tensor
    emax: int


def _fp6(ebits, mbits, bias) -> _Fp6:
    g = _minifloat_grid(ebits, mbits, bias)
    return _Fp6(g, (g[:-1] + g[1:]) * 0.5, torch.cat([g, -g]), int(math.log2(float(g[-1]))))


def _fp6_codes(v: torch.Tensor, f: _Fp6) -> torch.Tensor:
    """FP6 codes of v (clamped to the largest value, round to nearest, ties to the even code), sign in bit 5 - kept on
    values that round to zero, as by the gfx950 scaled convert.  _fp4_codes' comparisons against the grid's
    midpoints, from a table: a value on midpoint j has j midpoints below it and j + 1 at or below - the even one of
    the two is its code; off a midpoint the two counts agree."""
    a = v.abs().clamp(max=float(f.grid[-1])).contiguous()
    below, upto = torch.bucketize(a, f.mids), torch.bucketize(a, f.mids, right=True)
    return torch.where(below % 2 == 0, below, upto) | torch.signbit(v).to(torch.int64) << 5


MX_NAN = 255                # E8M0 byte of a block that held a NaN / Inf (OCP: NaN): all 32 channels decode to NaN


def _mx_exp(am: torch.Tensor, emax: int) -> torch.Tensor:
    """E8M0 scale byte: clamp(floor(log2 amax) - emax + 127, 0, 254); amax 0 / denormal -> exponent -127."""
    bits = am.float().contiguous().view(torch.int32).to(torch.int64)
    e = ((bits >> 23) & 0xFF) - 127
    e = torch.where(am > 0, e, torch.full_like(e, -127))
    return (e - emax + 127).clamp(0, 254)


def _e8m0(sb: torch.Tensor) -> torch.Tensor:
    v = (sb.to(torch.int64) << 23).to(torch.int32).view(torch.float32)
    return torch.where(sb == 0, torch.full_like(v, 2.0 ** -127), v)


_FP6 = {FMT_MXFP6: _fp6(2, 3, 1), FMT_MXBF6: _fp6(3, 2, 3)}      # E2M3: max 7.5, emax 2; E3M2: max 28, emax 4
_MX_EMAX = {FMT_MXFP4: 2, FMT_MXFP8: 8, FMT_MXFP6: _FP6[FMT_MXFP6].emax, FMT_MXBF6: _FP6[FMT_MXBF6].emax}


def _mx_pack(rows: torch.Tensor, fmt: int) -> torch.Tensor:
    n, H = rows.shape
    blk = rows.float().reshape(n, H // 32, 32)
    am = blk.abs().amax(-1)                                                  # NaN if the block holds one
    sb = _mx_exp(am, _MX_EMAX[fmt])                                          # [n, H/32]
    y = blk / _e8m0(sb)[..., None]
    sb = torch.where(torch.isfinite(am), sb, torch.full_like(sb, MX_NAN))    # codes of such a block: don't care
    if fmt == FMT_MXFP4:
        c = _fp4_codes(y).reshape(n, H // 2, 2)
        codes = (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8)
    elif fmt in MX6_FORMATS:   # 4 codes = 3 bytes of the block's little-endian 6-bit stream
        c = _fp6_codes(y, _FP6[fmt]).reshape(n, H // 4, 4)
        w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
        codes = torch.stack([w & 255, (w >> 8) & 255, w >> 16], -1).to(torch.uint8)
    else:
        codes = y.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).reshape(n, H)
    return torch.cat([codes.reshape(n, -1), sb.to(torch.uint8)], 1).reshape(-1)


def _mx_unpack(b: torch.Tensor, fmt: int, n: int, H: int) -> torch.Tensor:
    r = b.reshape(n, -1)
    nc = H // 2 if fmt == FMT_MXFP4 else 3 * H // 4 if fmt in MX6_FORMATS else H
    codes, sb = r[:, :nc], r[:, nc:].to(torch.int64)
    if fmt == FMT_MXFP4:
        c = torch.stack([codes & 15, codes >> 4], -1).reshape(n, H).to(torch.int64)
        v = _FP4_GRID[c & 7] * torch.where(c >= 8, -1.0, 1.0)
    elif fmt in MX6_FORMATS:
        b3 = codes.to(torch.int64).reshape(n, H // 4, 3)
        w = b3[..., 0] | (b3[..., 1] << 8) | (b3[..., 2] << 16)
        v = _FP6[fmt].values[torch.stack([(w >> (6 * e)) & 63 for e in range(4)], -1).reshape(n, H)]
    else:
        v = codes.contiguous().view(torch.float8_e4m3fn).float()
    out = v.reshape(n, H // 32, 32) * _e8m0(sb)[..., None]
    return torch.where((sb == MX_NAN)[..., None], torch.full_like(out, float("nan")), out).reshape(n, H)


# ---- NVFP4 rows (csrc/codec.hip nv_block / nv_pack8 / nv_unpack8) ---------------------------------------------
NV_BLOCK = 16               # channels per E4M3 scale


def _nv_step(sb: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """d = e4m3(sb) * g of scale bytes [n, H/16] and the rows' g [n]: one fp32 multiply."""
    return sb.contiguous().view(torch.float8_e4m3fn).float() * g[:, None]


def _nv_pack(rows: torch.Tensor) -> torch.Tensor:
    n, H = rows.shape
    blk = rows.float().reshape(n, H // NV_BLOCK, NV_BLOCK)
    g = rows.float().abs().amax(-1) / 2688.0                                 # NaN if the row holds one
    w = (blk.abs().amax(-1) / g[:, None]) / 6.0
    w = torch.where(w < 448.0, w, torch.full_like(w, 448.0))                 # the clamp; a NaN w takes 448 too
    sb = torch.where((g == 0)[:, None], torch.zeros_like(w), w).to(torch.float8_e4m3fn).view(torch.uint8)
    d = _nv_step(sb, g)
    c = _fp4_codes((blk / d[..., None]).clamp(-6.0, 6.0))
    c = torch.where(((sb == 0) | (d < 2.0 ** -126))[..., None], torch.zeros_like(c), c).reshape(n, H // 2, 2)
    return torch.cat([(c[..., 0] | (c[..., 1] << 4)).to(torch.uint8), sb, _bytes(g).reshape(n, 4)], 1).reshape(-1)


def _nv_unpack(b: torch.Tensor, n: int, H: int) -> torch.Tensor:
    r = b.reshape(n, -1)
    codes, sb, g = r[:, :H // 2], r[:, H // 2:H // 2 + H // NV_BLOCK], r[:, -4:].contiguous().view(torch.float32)[:, 0]
    c = torch.stack([codes & 15, codes >> 4], -1).reshape(n, H).to(torch.int64)
    v = _FP4_GRID[c & 7] * torch.where(c >= 8, -1.0, 1.0)
    out = (v.reshape(n, H // NV_BLOCK, NV_BLOCK) * _nv_step(sb, g)[..., None]).reshape(n, H)
    return torch.where(torch.isfinite(g)[:, None], out, torch.full_like(out, float("nan")))


def _grp_bits_pack(q: torch.Tensor, bits: int) -> torch.Tensor:
    """Codes [n, 64] (two's complement, |q| < 2^(bits-1)) -> the group's little-endian bit stream [n, 8 bits] bytes:
    code c at bits [bits c, bits c + bits); 8 consecutive codes are ``bits`` whole bytes (csrc/codec.hip grp_pack8)."""
    n = q.shape[0]
    c = (q.to(torch.int64) & ((1 << bits) - 1)).view(n, 8, 8)
    w = (c << (bits * torch.arange(8, dtype=torch.int64))).sum(-1)                      # [n, 8] words < 2^(8 bits)
    return ((w[..., None] >> (8 * torch.arange(bits, dtype=torch.int64))) & 255).to(torch.uint8).reshape(n, 8 * bits)


def _grp_bits_unpack(b: torch.Tensor, bits: int) -> torch.Tensor:
    n = b.shape[0]
    w = (b.to(torch.int64).view(n, 8, bits) << (8 * torch.arange(bits, dtype=torch.int64))).sum(-1)   # [n, 8]
    c = (w[..., None] >> (bits * torch.arange(8, dtype=torch.int64))) & ((1 << bits) - 1)
    c = torch.where(c >= (1 << (bits - 1)), c - (1 << bits), c)
    return c.reshape(n, 64).float()


def _wht64(v: torch.Tensor) -> torch.Tensor:
    """Unnormalised 64-point Walsh-Hadamard transform (Sylvester order) of the last dimension: the butterflies
    (a, b) -> (a + b, a - b) at channel strides 1, 2, 4, 8, 16, 32 in that order, in the tensor's own arithmetic
    (fp32 adds on encode, integer adds on decode) - the order and operations of csrc/codec.hip wht8 / wht_lanes."""
    lead = v.shape[:-1]
    for h in (1, 2, 4, 8, 16, 32):
        p = v.reshape(*lead, GROUP // (2 * h), 2, h)
        a, b = p[..., 0, :], p[..., 1, :]
        v = torch.stack((a + b, a - b), -2).reshape(*lead, GROUP)
    return v


def _wht32(v: torch.Tensor) -> torch.Tensor:
    """Unnormalised 32-point Walsh-Hadamard transform (Sylvester order) of the last dimension in fp32: the butterflies
    (a, b) -> (a + b, a - b) at channel strides 1, 2, 4, 8, 16 in that order, the lower index keeping the sum - the
    order and operations of csrc/codec.hip wht8 / wht_quad (4 and 8-bit rows) and wht32 (6-bit rows)."""
    lead = v.shape[:-1]
    for h in (1, 2, 4, 8, 16):
        p = v.reshape(*lead, 32 // (2 * h), 2, h)
        a, b = p[..., 0, :], p[..., 1, :]
        v = torch.stack((a + b, a - b), -2).reshape(*lead, 32)
    return v


def _rot32(rows: torch.Tensor, scale: float) -> torch.Tensor:
    """``scale`` H32 x of every 32-channel block of fp32 rows [n, H]: 0.25 before the quantizer, 0.125 after the
    dequantizer (both exact multiplies, after the last add)."""
    n, H = rows.shape
    return (_wht32(rows.float().reshape(n, H // 32, 32)) * scale).reshape(n, H)


def _wht128(v: torch.Tensor) -> torch.Tensor:
    """Unnormalised 128-point Walsh-Hadamard transform (Sylvester order) of the last dimension in fp32: the butterflies
    (a, b) -> (a + b, a - b) at channel strides 1, 2, 4, 8, 16, 32, 64 in that order, the lower index keeping the sum -
    the order and operations of csrc/codec.hip wht_row16."""
    lead = v.shape[:-1]
    for h in (1, 2, 4, 8, 16, 32, 64):
        p = v.reshape(*lead, 128 // (2 * h), 2, h)
        a, b = p[..., 0, :], p[..., 1, :]
        v = torch.stack((a + b, a - b), -2).reshape(*lead, 128)
    return v


def _rot128(rows: torch.Tensor, scale) -> torch.Tensor:
    """``scale`` H128 x of every 128-channel block of fp32 rows [n, H]: 0.125 before the quantizer, the rows' s / 16
    ([n, 1, 1]) on the decoder's integer sums (one multiply, after the last add)."""
    n, H = rows.shape
    return (_wht128(rows.float().reshape(n, H // 128, 128)) * scale).reshape(n, H)


@lru_cache(maxsize=1)
def _h28() -> torch.Tensor:
    """The Paley type II Hadamard matrix of order 28 (q = 13), fp32 [28, 28], symmetric: Q[i][j] = chi(i - j) with chi
    the quadratic character mod 13, C = [[0, 1'], [1, Q]] (14 x 14), H28 = C (x) [[1, 1], [1, -1]] + I14 (x) [[1, -1],
    [-1, -1]] - the formula of csrc/codec.hip make_h28."""
    squares = {k * k % 13 for k in range(1, 13)}
    chi = [0] + [1 if r in squares else -1 for r in range(1, 13)]
    C = torch.ones(14, 14)
    C[0, 0] = 0.0
    C[1:, 1:] = torch.tensor([[float(chi[(i - j) % 13]) for j in range(13)] for i in range(13)])
    return torch.kron(C, torch.tensor([[1.0, 1.0], [1.0, -1.0]])) + \
        torch.kron(torch.eye(14), torch.tensor([[1.0, -1.0], [-1.0, -1.0]]))


def _wht_last(v: torch.Tensor) -> torch.Tensor:
    """Unnormalised Walsh-Hadamard transform (Sylvester order) of the last dimension, a power of two, in fp32: the
    butterflies (a, b) -> (a + b, a - b) at strides 1, 2, ... in that order, the lower index keeping the sum."""
    lead, n, h = v.shape[:-1], v.shape[-1], 1
    while h < n:
        p = v.reshape(*lead, n // (2 * h), 2, h)
        a, b = p[..., 0, :], p[..., 1, :]
        v, h = torch.stack((a + b, a - b), -2).reshape(*lead, n), 2 * h
    return v


def _h28_stage(t: torch.Tensor) -> torch.Tensor:
    """out[:, a'] = sum_a H28[a'][a] t[:, a] of fp32 [n, 28, W], accumulated in ascending a from +-t[:, 0] - the order
    is the format's (csrc/codec.hip h28_dot)."""
    Hm = _h28()
    acc = Hm[:, 0, None] * t[:, 0:1, :]
    for a in range(1, 28):
        acc = acc + Hm[:, a, None] * t[:, a:a + 1, :]     # +-1 times t is exact: an add or a subtract of t[a]
    return acc


def _full_scales(H: int):
    """(e, d) of a whole-row rotation: the encoder's y = e H x and the decoder's x' = (s d) H q.  H = 2^n: 2^-floor(n/2),
    2^-ceil(n/2).  H = 28 * 2^m: 2^-(2 + floor(m/2)), fp32(1/28) 2^(2 + floor(m/2) - m)."""
    if H & (H - 1) == 0:
        n = H.bit_length() - 1
        return 2.0 ** -(n // 2), torch.tensor(2.0 ** -((n + 1) // 2))
    m = (H // 28).bit_length() - 1
    return 2.0 ** -(2 + m // 2), (torch.ones(()) / 28.0) * 2.0 ** (2 + m // 2 - m)


def _rot_full(rows: torch.Tensor, decode_scale: torch.Tensor | None = None) -> torch.Tensor:
    """The whole-row rotation of fp32 rows [n, H], H in ROW_ROT_FULL_SIZES (channel a 2^m + b, H = H28 (x) H_2^m, or
    the Sylvester matrix of order H).  Encoder (``decode_scale`` None): the Sylvester stages, the 28-point stage, one
    multiply by e.  Decoder: the 28-point stage, the Sylvester stages, one multiply by ``decode_scale`` (the rows'
    fp32 s d, [n])."""
    n, H = rows.shape
    e, _ = _full_scales(H)
    v = rows.float()
    if H & (H - 1):
        v = v.reshape(n, 28, H // 28)
        v = _wht_last(_h28_stage(v)) if decode_scale is not None else _h28_stage(_wht_last(v))
        v = v.reshape(n, H)
    else:
        v = _wht_last(v)
    return v * (e if decode_scale is None else decode_scale[:, None])


def hadamard64(x: torch.Tensor) -> torch.Tensor:
    """y_g = H64 x_g / 8 for every 64-channel group of fp32 rows [n, H]: orthonormal, symmetric, its own inverse.
    The scaling by 1/8 is exact, so the only roundings are those of the 6 butterfly levels' fp32 adds."""
    n, H = x.shape
    return (_wht64(x.float().reshape(n, H // GROUP, GROUP)) * 0.125).reshape(n, H)


def _grp_quant(blk: torch.Tensor, bits: int):
    """The quantizer of one 64-channel group of fp32 rows [n, 64] at ``bits``: (codes q [n, 64] as floats, scales s
    [n]) with s = max|x| / qmax (qmax = 2^(bits-1) - 1) and q = clamp(round(x * (1 / s)), -qmax, qmax), 1 / s taken
    as 0 for an all-zero group (csrc/codec.hip grp_quant / grp_q); the decoder returns q * s."""
    qmax = (1 << (bits - 1)) - 1
    am = blk.abs().amax(-1)
    s = am / float(qmax)
    inv = torch.where(am > 0, 1.0 / torch.where(am > 0, s, torch.ones_like(s)), torch.zeros_like(s))
    return torch.round(blk * inv[:, None]).clamp(-qmax, qmax), s


def _grp_pack(rows: torch.Tensor, plan, rot: bool = False) -> torch.Tensor:
    """FMT_GRP rows: per 64-channel group g of b_g bits, s = max|x| / qmax_b (qmax = 2^(b-1) - 1), codes
    clamp(round(x * (1 / s)), -qmax, qmax) packed as a b-bit stream (csrc/codec.hip grp_pack8); then the G fp32
    scales.  ``rot`` (FMT_GRPR): the same of the rotated groups ``hadamard64(rows)``."""
    n, H = rows.shape
    if rot:
        rows = hadamard64(rows)
    parts, scales = [], []
    for g, b in enumerate(plan):
        q, s = _grp_quant(rows[:, g * GROUP:(g + 1) * GROUP].float(), b)
        parts.append(_grp_bits_pack(q, b))
        scales.append(s)
    sc = torch.stack(scales, 1).contiguous().view(torch.uint8).reshape(n, -1)
    return torch.cat(parts + [sc], 1).reshape(-1)


def _grp_unpack(b: torch.Tensor, msg_plan, plan, n: int, rot: bool = False) -> torch.Tensor:
    """FMT_GRP / FMT_GRPR rows -> fp32 [n, H].  The row stride comes from the codec's plan, the widths from the
    MESSAGE's plan bytes as on the GPU (csrc/codec.hip grp_walk): a width outside GROUP_BITS, or a group stream
    reaching past the row's code bytes, gives NaN from that group on (invalid widths count 0 bytes in the offset).
    ``rot`` (FMT_GRPR): the group's integer codes go through the butterflies as integers (exact) and one multiply by
    s / 8 gives x' = H64 q s / 8."""
    r = b.reshape(n, -1)
    cb = sum(8 * x for x in plan)
    sc = r[:, cb:].contiguous().view(torch.float32).reshape(n, len(plan))
    out, off, bad = [], 0, False
    for g, bits in enumerate(msg_plan):
        ok = bits in GROUP_BITS
        bad = bad or not ok or off + 8 * bits > cb
        if bad:
            out.append(torch.full((n, GROUP), float("nan")))
        else:
            q = _grp_bits_unpack(r[:, off:off + 8 * bits].contiguous(), bits)
            out.append(_wht64(q.to(torch.int64)).float() * (sc[:, g:g + 1] * 0.125) if rot else q * sc[:, g:g + 1])
        off += 8 * bits if ok else 0
    return torch.cat(out, 1)


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8).reshape(-1)


# ---- scaled fp16 rows (csrc/codec.hip f16s_scale / f16_store8 / f16_load8) ---------------------------------------
def _f16s_scale(am: torch.Tensor):
    """(p, inv) [n] of FMT_F16S rows from their max-abs ``am`` (NaN if the row holds one), built from integer bit
    patterns as the kernel does: p = 2^k, inv = 2^-k, k = clamp(E - 141, -112, 113) with E the biased exponent field
    of am; am = 0 -> 1, 1; am NaN / Inf -> am, 1."""
    bits = am.float().contiguous().view(torch.int32).to(torch.int64) & 0x7FFFFFFF
    E = bits >> 23
    k = (E - 141).clamp(-112, 113)
    p = ((127 + k) << 23).to(torch.int32).view(torch.float32)
    inv = ((127 - k) << 23).to(torch.int32).view(torch.float32)
    one = torch.ones_like(p)
    p, inv = torch.where(bits == 0, one, p), torch.where(bits == 0, one, inv)
    return torch.where(E == 255, am.float(), p), torch.where(E == 255, one, inv)


def _f16s_pack(rows: torch.Tensor) -> torch.Tensor:
    n = rows.shape[0]
    p, inv = _f16s_scale(rows.abs().amax(-1))
    codes = (rows * inv[:, None]).to(torch.float16)
    return torch.cat([codes.contiguous().view(torch.uint8).reshape(n, -1),
                      p.contiguous().view(torch.uint8).reshape(n, 4)], 1).reshape(-1)


def _f16s_unpack(raw: torch.Tensor, n: int, H: int) -> torch.Tensor:
    r = raw.reshape(n, 2 * H + 4)
    p = r[:, 2 * H:].contiguous().view(torch.float32)                     # [n, 1]
    return r[:, :2 * H].contiguous().view(torch.float16).float() * p


@dataclass(frozen=True)
class RowCtx:
    """What a row format's CPU pack / unpack may need beyond the rows of one class."""
    H: int
    plan: tuple | None                 # the codec's group bit plan (row stride)
    msg_plan: list | None              # the plan bytes as the message holds them (widths, when decoding)
    spec: CodecSpec
    is_lo: bool
    scale_row: torch.Tensor | None     # [n] per-row scale of the class's rows (token / window modes)
    ch_scale: torch.Tensor | None      # [n, H] per-channel scale of the class's rows (channel mode)


@dataclass(frozen=True)
class RowFormat:
    """One row format of the wire."""
    row_bytes: Callable[[int, tuple | None], int]                   # (H, plan) -> bytes of one row
    self_scaled: bool          # no entry in the message's scale section (csrc/codec.hip SELF_SCALED)
    pack: Callable[[torch.Tensor, RowCtx], torch.Tensor]            # (fp32 rows [n, H], ctx) -> the rows' bytes
    unpack: Callable[[torch.Tensor, int, RowCtx], torch.Tensor]     # (bytes, n, ctx) -> fp32 rows [n, H]


def _row_rotated(rows: torch.Tensor, rot) -> torch.Tensor:
    """What a rotated twin quantizes: y = H128 x / 8 of every block (``rot`` True) or y = e H x of the row ("full")."""
    return _rot_full(rows) if rot == "full" else _rot128(rows, 0.125)


def _int_rows(fmt: int, per_byte: int, rot=False) -> RowFormat:
    """``rot``: a rotated twin (SC_TOKEN only) - the same bytes of y = H128 x / 8 (True) or of the whole row's y = e H x
    ("full"), whose max-abs made c.scale_row (_encode_cpu); the decoder rotates the integer codes back and multiplies
    once, by s / 16 or s d."""
    def pack(rows, c):
        return _pack_rows(_qcodes(_row_rotated(rows, rot) if rot else rows, c.spec, c.is_lo, c.scale_row, c.ch_scale),
                          fmt)

    def unpack(raw, n, c):
        if rot == "full":
            return _rot_full(_unpack_rows(raw, fmt, n, c.H), c.scale_row * _full_scales(c.H)[1])
        if rot:
            return _rot128(_unpack_rows(raw, fmt, n, c.H), (c.scale_row * 0.0625)[:, None, None])
        return _dequant(_unpack_rows(raw, fmt, n, c.H), c.spec, c.is_lo, c.scale_row, c.ch_scale)
    return RowFormat(lambda H, plan: H // per_byte, False, pack, unpack)


def _top8(rows: torch.Tensor):
    """The outliers of fp32 rows [n, H]: (channels [n, 8] int64, values [n, 8] fp32, the rows with those channels +0).
    One topk over the unique keys abs_bits << 32 | (2^32 - 1 - channel): descending magnitude on the bit pattern of
    |x| (NaN > Inf > finite), ties to the lower channel (csrc/codec.hip out_extract)."""
    n, H = rows.shape
    ab = rows.contiguous().view(torch.int32).to(torch.int64) & 0x7FFFFFFF
    idx = torch.topk((ab << 32) | (0xFFFFFFFF - torch.arange(H, dtype=torch.int64)), OUT_K, dim=1).indices
    return idx, rows.gather(1, idx), rows.scatter(1, idx, 0.0)


def _out_rows(fmt: int, per_byte: int) -> RowFormat:
    """The outlier twin of int format ``fmt``: [fmt's codes of the rest][8 fp32 values][8 uint16 channels]; the row's
    scale (c.scale_row: max|rest| / qmax, _encode_cpu) is in the message's scale section as for ``fmt``."""
    def pack(rows, c):
        idx, val, rest = _top8(rows)
        codes = _pack_rows(_qcodes(rest, c.spec, c.is_lo, c.scale_row, c.ch_scale), fmt).reshape(len(rows), -1)
        return torch.cat([codes, val.contiguous().view(torch.uint8).reshape(len(rows), -1),
                          idx.to(torch.int16).view(torch.uint8).reshape(len(rows), -1)], 1).reshape(-1)

    def unpack(raw, n, c):
        r, nc = raw.reshape(n, -1), c.H // per_byte
        out = _dequant(_unpack_rows(r[:, :nc].reshape(-1), fmt, n, c.H), c.spec, c.is_lo, c.scale_row, c.ch_scale)
        val = r[:, nc:nc + 4 * OUT_K].contiguous().view(torch.float32)
        idx = r[:, nc + 4 * OUT_K:].contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
        for p in range(OUT_K):          # in pair order: of two pairs naming one channel the last holds
            out[torch.arange(n), idx[:, p].clamp(max=c.H - 1)] = val[:, p]
        out[(idx >= c.H).any(1)] = float("nan")
        return out
    return RowFormat(lambda H, plan: H // per_byte + OUT_TAIL, False, pack, unpack)


def _mx_rows(fmt: int, code_bits: int, rot: bool = False) -> RowFormat:    # codes, then one E8M0 byte per 32 channels
    """``rot``: the rotated twin - the same bytes of the blocks rotated before the pack and back after the unpack."""
    if rot:
        return RowFormat(lambda H, plan: H * code_bits // 8 + H // 32, True,
                         lambda rows, c: _mx_pack(_rot32(rows, 0.25), fmt),
                         lambda raw, n, c: _rot32(_mx_unpack(raw, fmt, n, c.H), 0.125))
    return RowFormat(lambda H, plan: H * code_bits // 8 + H // 32, True,
                     lambda rows, c: _mx_pack(rows, fmt), lambda raw, n, c: _mx_unpack(raw, fmt, n, c.H))


def _grp_rows(rot: bool) -> RowFormat:   # codes of every group (8 * bits bytes), then one fp32 scale per group
    return RowFormat(lambda H, plan: sum(8 * b for b in plan) + 4 * len(plan), True,
                     lambda rows, c: _grp_pack(rows, c.plan, rot),
                     lambda raw, n, c: _grp_unpack(raw, c.msg_plan, c.plan, n, rot))


ROW_FORMATS = {
    FMT_BF16: RowFormat(lambda H, plan: 2 * H, True, lambda rows, c: _bytes(rows.to(torch.bfloat16)),
                        lambda raw, n, c: raw.view(torch.bfloat16).reshape(n, c.H).float()),
    FMT_F32: RowFormat(lambda H, plan: 4 * H, True, lambda rows, c: _bytes(rows),
                       lambda raw, n, c: raw.view(torch.float32).reshape(n, c.H)),
    FMT_INT8: _int_rows(FMT_INT8, 1), FMT_INT4: _int_rows(FMT_INT4, 2), FMT_INT2: _int_rows(FMT_INT2, 4),
    FMT_INT8O: _out_rows(FMT_INT8, 1), FMT_INT4O: _out_rows(FMT_INT4, 2), FMT_INT2O: _out_rows(FMT_INT2, 4),
    FMT_INT8R: _int_rows(FMT_INT8, 1, True), FMT_INT4R: _int_rows(FMT_INT4, 2, True),
    FMT_INT2R: _int_rows(FMT_INT2, 4, True),
    FMT_INT8F: _int_rows(FMT_INT8, 1, "full"), FMT_INT4F: _int_rows(FMT_INT4, 2, "full"),
    FMT_INT2F: _int_rows(FMT_INT2, 4, "full"),
    FMT_MXFP4: _mx_rows(FMT_MXFP4, 4), FMT_MXFP8: _mx_rows(FMT_MXFP8, 8),
    FMT_MXFP6: _mx_rows(FMT_MXFP6, 6), FMT_MXBF6: _mx_rows(FMT_MXBF6, 6),
    FMT_MXFP4R: _mx_rows(FMT_MXFP4, 4, True), FMT_MXFP8R: _mx_rows(FMT_MXFP8, 8, True),
    FMT_MXFP6R: _mx_rows(FMT_MXFP6, 6, True), FMT_MXBF6R: _mx_rows(FMT_MXBF6, 6, True),
    FMT_NVFP4: RowFormat(lambda H, plan: 9 * H // 16 + 4, True, lambda rows, c: _nv_pack(rows),
                         lambda raw, n, c: _nv_unpack(raw, n, c.H)),
    FMT_GRP: _grp_rows(False), FMT_GRPR: _grp_rows(True),
    FMT_F16: RowFormat(lambda H, plan: 2 * H, True, lambda rows, c: _bytes(rows.to(torch.float16)),
                       lambda raw, n, c: raw.view(torch.float16).reshape(n, c.H).float()),
    FMT_F16S: RowFormat(lambda H, plan: 2 * H + 4, True, lambda rows, c: _f16s_pack(rows),
                        lambda raw, n, c: _f16s_unpack(raw, n, c.H)),
}


def _fmt_word(spec: CodecSpec, L: Layout) -> int:
    """Header word 7: the hi-row format; with 6-bit or rotated MX rows, outlier rows or rotated int rows (with_mx_elem,
    with_mx_rot, with_outliers, with_row_rot) the lo-row format too, in bits 8-15."""
    both = spec.mx_elem != FMT_MXFP4 or spec.mx_rot or spec.outliers or spec.row_rot
    return L.hi_fmt | L.lo_fmt << 8 if both else L.hi_fmt


def _header(spec: CodecSpec, L: Layout) -> torch.Tensor:
    return torch.tensor([MAGIC, VERSION, spec.cid, L.B, L.S, L.H, -1 if L.kvar else L.k, _fmt_word(spec, L)],
                        dtype=torch.int32)


def _check_formats(spec: CodecSpec, L: Layout, msg: torch.Tensor | None = None) -> None:
    """decode's refusal of a message whose row formats are not the spec's: the layout's against the spec with its
    modifiers (any device, no read of the message), and the header's format word of a CPU message against the
    layout's.  (The GPU kernels check the word of a message with 6-bit or rotated MX rows themselves and decode it to
    NaN.)"""
    for name, got, fmt in (("hi", L.hi_fmt, spec.hi_fmt), ("lo", L.lo_fmt, spec.lo_fmt)):
        want = (got if spec.native_wire == NATIVE and got in (FMT_BF16, FMT_F32) else spec.native_wire) \
            if fmt == NATIVE else _resolve(fmt, spec, NATIVE)
        if got != want:
            raise ValueError(f"codec {spec.name}: the message's {name} rows have format {got}, the spec's {want}")
    if msg is not None and int(msg[28:32].view(torch.int32)) != _fmt_word(spec, L):
        raise ValueError(f"codec {spec.name}: header format word {int(msg[28:32].view(torch.int32))}, "
                         f"the spec's {_fmt_word(spec, L)}")


def _classes(spec, L, lo_mask, scales, msg_plan):
    """Per class with rows, hi first: (row format, selection [B, S], message offset, RowCtx of the selection)."""
    kt = int(lo_mask.sum())
    for is_lo, fmt in ((False, L.hi_fmt), (True, L.lo_fmt)):
        sel = lo_mask if is_lo else ~lo_mask
        if not bool(sel.any()):
            continue
        srow = ch = None
        if spec.scale_mode == SC_CHANNEL:
            ch = scales.view(L.B, 1, L.H).expand(L.B, L.S, L.H)[sel]
        elif spec.scale_mode != SC_NONE:
            srow = (scales if spec.scale_mode == SC_TOKEN else scales.view(L.B, 1).expand(L.B, L.S))[sel]
        yield (ROW_FORMATS[fmt], sel, L.off_lo if is_lo else L.hi_offset(kt),
               RowCtx(L.H, L.plan, msg_plan, spec, is_lo, srow, ch))


def _encode_cpu(x, spec, L, lo_mask):
    B, S, H = L.B, L.S, L.H
    msg = torch.zeros(L.total, dtype=torch.uint8)

    def put(off, t):
        data = _bytes(t)
        msg[off:off + data.numel()] = data

    put(0, _header(spec, L))
    put(L.off_mask, _mask_words(lo_mask, L.mw))
    if L.kvar:
        put(L.off_kvec, lo_mask.sum(1).to(torch.int32))
    if L.plan is not None:
        put(L.off_plan, torch.tensor(L.plan, dtype=torch.uint8))
    xf = x.float().reshape(B, S, H)
    # statistics
    scales = None
    if spec.scale_mode == SC_TOKEN:
        scales = torch.zeros(B, S)
        for is_lo, fmt, qmax in ((False, L.hi_fmt, spec.qmax_hi), (True, L.lo_fmt, spec.qmax_lo)):
            if not ROW_FORMATS[fmt].self_scaled:   # an outlier row: the max-abs of what its 8 outliers leave;
                rows = xf.reshape(B * S, H)        # a rotated row: that of y = H128 x / 8, or of the row's y = e H x
                am = (_top8(rows)[2].reshape(B, S, H) if fmt in OUT_TWIN.values() else
                      _rot128(rows, 0.125).reshape(B, S, H) if fmt in ROW_ROT_TWIN.values() else
                      _rot_full(rows).reshape(B, S, H) if fmt in ROW_ROT_FULL_TWIN.values() else xf).abs().amax(-1)
                scales = torch.where(lo_mask if is_lo else ~lo_mask, am / float(qmax), scales)
    elif spec.scale_mode == SC_WINDOW:
        scales = torch.where(lo_mask[..., None], xf.abs(), torch.zeros_like(xf)).amax(dim=(1, 2))
    elif spec.scale_mode == SC_CHANNEL:
        scales = xf.abs().amax(1) if spec.ch_kind == CH_MAXABS else xf.mean(1) + 1e-8   # [B, H]
    if scales is not None:
        put(L.off_scale, scales)
    # rows, in window/token order
    for rf, sel, off, c in _classes(spec, L, lo_mask, scales, L.plan):
        put(off, rf.pack(xf[sel], c))
    return msg


def _decode_cpu(msg, spec, L, dtype):
    B, S, H = L.B, L.S, L.H
    words = msg[L.off_mask:L.off_mask + B * L.mw * 4].view(torch.int32).reshape(B, L.mw)
    lo_mask = _words_to_mask(words, S)
    out = torch.empty(B, S, H, dtype=torch.float32)
    shape = _scale_shape(spec.scale_mode, B, S, H)
    scales = None if shape is None else \
        msg[L.off_scale:L.off_scale + 4 * math.prod(shape)].view(torch.float32).reshape(shape)
    msg_plan = None if L.plan is None else msg[L.off_plan:L.off_plan + len(L.plan)].tolist()
    for rf, sel, off, c in _classes(spec, L, lo_mask, scales, msg_plan):
        n = int(sel.sum())
        out[sel] = rf.unpack(msg[off:off + n * rf.row_bytes(H, L.plan)], n, c)
    return out.reshape(B * S, H).to(dtype)


# --------------------------------------------------------------------------------------------
# GPU implementation
_DEV_CONSTS: dict = {}


def _dev_const(key, device, make):
    """A small constant tensor (header, plan bytes) on ``device``, uploaded once."""
    t = _DEV_CONSTS.get((key, device))
    if t is None:
        t = _DEV_CONSTS[(key, device)] = make().to(device)
    return t


def _args(spec, L):
    gcb = sum(8 * b for b in L.plan) if L.plan is not None else 0
    return (L.off_mask, L.off_scale, L.off_hi, L.off_lo, L.off_kvec, L.off_plan, L.B, L.S, L.H, max(L.k, 0),
            L.hi_fmt, L.lo_fmt, spec.scale_mode, spec.qmax_hi, spec.qmax_lo, spec.ch_kind, gcb)


def _encode_gpu(x, spec, L, imp, msg, mass=0.0):
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("GPU boundary codec expects bf16 or fp32 activations")
    xf32 = int(x.dtype == torch.float32)
    st = stream()
    msg[:32].copy_(_dev_const(("header", spec.cid, L), x.device, lambda: _header(spec, L).view(torch.uint8)))
    if L.plan is not None:
        msg[L.off_plan:L.off_plan + len(L.plan)].copy_(
            _dev_const(("plan", L.plan), x.device, lambda: torch.tensor(L.plan, dtype=torch.uint8)))
    if L.kvar:
        if imp is None:
            raise ValueError("top-rho selection needs token importance")
        call("edge_select", ptr(imp.float().contiguous()), L.B, L.S, 0, ptr(msg), L.off_mask, 1, float(mass),
             L.off_kvec, st)
    elif 0 < L.k < L.S:
        if imp is None:
            raise ValueError(f"codec {spec.name} with 0 < k < S needs token importance")
        call("edge_select", ptr(imp.float().contiguous()), L.B, L.S, L.k, ptr(msg), L.off_mask, 0, 0.0, -1, st)
    else:
        call("edge_set_mask", ptr(msg), L.off_mask, L.B, L.S, 1 if L.k >= L.S else 0, st)
    if spec.scale_mode == SC_WINDOW:
        tmp = torch.empty(L.B, L.H, dtype=torch.float32, device=x.device)
        call("edge_channel_stats", ptr(x), ptr(msg), L.off_mask, ptr(tmp), L.B, L.S, L.H, CH_MAXABS, 1, xf32, st)
        call("edge_rowmax", ptr(tmp), msg.data_ptr() + L.off_scale, L.B, L.H, st)
    elif spec.scale_mode == SC_CHANNEL:
        call("edge_channel_stats", ptr(x), ptr(msg), L.off_mask, msg.data_ptr() + L.off_scale, L.B, L.S, L.H,
             spec.ch_kind, 0, xf32, st)
    call("edge_pack", ptr(x), ptr(msg), *_args(spec, L), xf32, st)
    return msg


def _decode_gpu(msg, spec, L, out):
    if out.dtype not in (torch.bfloat16, torch.float32) or not out.is_contiguous():
        raise TypeError("GPU boundary codec decodes into contiguous bf16 or fp32 activations")
    call("edge_unpack", ptr(out), ptr(msg), *_args(spec, L), int(out.dtype == torch.float32), stream())
    return out


# --------------------------------------------------------------------------------------------
SELECTIONS = ("ratio", "top_rho")


def uses_kvar(spec: CodecSpec, selection: str) -> bool:
    if selection not in SELECTIONS:
        raise ValueError(f"unknown selection {selection!r}; known: {SELECTIONS}")
    return selection == "top_rho" and spec.uses_ratio


def encode(x: torch.Tensor, spec: CodecSpec, B: int, S: int, ratio: float = 0.0, importance=None,
           out: torch.Tensor | None = None, k: int | None = None,
           selection: str = "ratio") -> tuple[torch.Tensor, Layout]:
    """Quantize and pack ``x`` ([B*S, H]) into one boundary message (uint8 tensor).

    ``selection="ratio"``: the lo class is the ``k = int(ratio*S)`` least important tokens (``k`` may be given
    directly).  ``"top_rho"``: every window keeps its shortest descending-importance prefix reaching mass
    ``1 - ratio`` and quantizes the rest (per-window k, variable-k message)."""
    H = x.shape[-1]
    kvar, mass = uses_kvar(spec, selection), 1.0 - float(ratio)
    if kvar:
        if importance is None:
            if mass > 0:
                raise ValueError("top-rho selection needs token importance")
            # ratio >= 1: keep mass <= 0 keeps nothing for any importance (every window all lo, k = S)
            importance = torch.zeros(B, S, dtype=torch.float32, device=x.device)
        L = layout(spec, B, S, H, -1, x.dtype, kvar=True)
    else:
        k = num_lo(spec, ratio, S) if k is None else (k if spec.uses_ratio else 0)
        L = layout(spec, B, S, H, k, x.dtype)
    if x.is_cuda:
        if out is None:  # zero-filled so the 16-byte section padding is deterministic on the wire
            out = torch.zeros(L.total, dtype=torch.uint8, device=x.device)
        return _encode_gpu(x.contiguous(), spec, L, importance, out, mass if kvar else 0.0), L
    if kvar:
        lo = select_mask(importance, top_rho_k(importance, mass))
    elif 0 < k < S:
        lo = select_mask(importance.float(), k)
    else:
        lo = torch.full((B, S), k >= S and k > 0, dtype=torch.bool)
    msg = _encode_cpu(x, spec, L, lo)
    if out is None:
        return msg, L
    out.copy_(msg)
    return out, L


def decode(msg: torch.Tensor, spec: CodecSpec, L: Layout, dtype=torch.bfloat16, out=None) -> torch.Tensor:
    """Unpack and dequantize a boundary message into ``[B*S, H]`` activations."""
    _check_formats(spec, L, None if msg.is_cuda else msg)
    if msg.is_cuda:
        if out is None:
            out = torch.empty(L.B * L.S, L.H, dtype=dtype, device=msg.device)
        return _decode_gpu(msg, spec, L, out)
    y = _decode_cpu(msg, spec, L, dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


def fake_quant(x: torch.Tensor, spec: CodecSpec, B: int, S: int, ratio: float = 0.0, importance=None,
               k: int | None = None, selection: str = "ratio"):
    """decode(encode(x)): what the receiving stage sees.  Returns (x_hat, message bytes)."""
    msg, L = encode(x, spec, B, S, ratio, importance, k=k, selection=selection)
    return decode(msg, spec, L, x.dtype), message_payload(msg, L)


def message_k(msg: torch.Tensor, L: Layout) -> torch.Tensor:
    """Per-window lo counts of a message [B] (reads the k vector of a variable-k message)."""
    if not L.kvar:
        return torch.full((L.B,), L.k, dtype=torch.int64)
    return msg[L.off_kvec:L.off_kvec + 4 * L.B].view(torch.int32).to(torch.int64)


def message_payload(msg: torch.Tensor, L: Layout) -> int:
    """Bytes a link carries for this message (host sync for a variable-k message)."""
    return L.total if not L.kvar else L.payload_bytes(int(message_k(msg, L).sum()))


# --------------------------------------------------------------------------------------------
# Fork: one hidden state -> the receiver-side activations of all (source, k) variants of one codec, stacked
FORK_MAXV = 64              # variants per launch (csrc/codec.hip FORK_MAXV); longer lists are split here
_FORK_ROWS = ((NATIVE, 0), (FMT_INT8, 127), (FMT_INT4, 7), (FMT_INT2, 1))


def fork_supported(spec: CodecSpec, selection: str = "ratio") -> bool:
    """``fake_quant_fork`` serves this codec: native / int8 / int4 / int2 rows with per-token or per-window scales,
    fixed k, NATIVE rows in the activation dtype (the codecs the sweeps run: ref_int4_global, int4_token, int8_token,
    int8_token_keep, mixed_int4_int8, mixed_int2_int8).  Everything else keeps the per-variant ``fake_quant``."""
    uses_kvar(spec, selection)       # an unknown selection: ValueError
    return (selection == "ratio" and spec.native_wire == NATIVE and spec.mx_elem == FMT_MXFP4 and not spec.mx_rot
            and not spec.outliers and not spec.row_rot
            and spec.scale_mode in (SC_TOKEN, SC_WINDOW)
            and (spec.hi_fmt, spec.qmax_hi) in _FORK_ROWS and (spec.lo_fmt, spec.qmax_lo) in _FORK_ROWS)


def _fork_gpu(x, spec, B, S, variants, importances, out):
    H, dev, nsrc = x.shape[-1], x.device, len(importances)
    L = layout(spec, B, S, H, 0, x.dtype)             # the resolved row formats
    imp = None
    if nsrc:
        imp = importances[0] if nsrc == 1 else torch.stack([i.reshape(B, S) for i in importances])
        imp = imp.float().contiguous()
    window = spec.scale_mode == SC_WINDOW
    rank = torch.empty(max(nsrc, 1) * B * S, dtype=torch.int32, device=dev) if nsrc or window else None
    amax = torch.empty(B * S, dtype=torch.int32, device=dev) if window else None
    for v0 in range(0, len(variants), FORK_MAXV):
        vs = tuple(variants[v0:v0 + FORK_MAXV])
        tab = _dev_const(("fork_tab", vs), dev, lambda: torch.tensor(vs, dtype=torch.int32))
        wscale = torch.empty(len(vs) * B, dtype=torch.float32, device=dev) if window else None
        call("edge_fake_quant_fork", ptr(x), ptr(out[v0 * B * S:]), ptr(imp), nsrc, ptr(tab), len(vs), ptr(rank),
             ptr(amax), ptr(wscale), B, S, H, L.hi_fmt, L.lo_fmt, spec.scale_mode, spec.qmax_hi, spec.qmax_lo,
             int(x.dtype == torch.float32), stream())
    return out


def fake_quant_fork(x: torch.Tensor, spec: CodecSpec, B: int, S: int, variants, importances=(), out=None):
    """``fake_quant`` of ``x`` ([B*S, H]) for every variant at once: (x_hat [V*B*S, H], message bytes per variant).

    ``variants``: a list of ``(source, k)`` - the lo class of variant v is the ``k`` least important tokens of every
    window by ``importances[source]`` ([B, S]); ``source`` None needs ``k`` in {0, S} (no importance read, as for any
    variant with such a ``k``).  Rows ``[v*B*S, (v+1)*B*S)`` of the result are bit for bit
    ``fake_quant(x, spec, B, S, importance=importances[source], k=k)[0]``, which is what runs for CPU tensors; CUDA
    tensors run one sort per source, one read of ``x`` and one write per variant (csrc/codec.hip fork_kernel) with no
    message in between.  ``out``: a contiguous [V*B*S, H] tensor of ``x``'s dtype to write into."""
    if not fork_supported(spec):
        raise ValueError(f"codec {spec.name} (native wire {spec.native_wire}) is not served by fake_quant_fork")
    H, V = x.shape[-1], len(variants)
    vs = []
    for src, k in variants:
        k = max(0, min(S, int(k))) if spec.uses_ratio else 0
        if 0 < k < S and src is None:
            raise ValueError(f"codec {spec.name} with 0 < k < S needs token importance")
        if src is not None and not 0 <= src < len(importances):
            raise ValueError(f"variant source {src} outside the {len(importances)} importances")
        vs.append((src, k))
    nbytes = [layout(spec, B, S, H, k, x.dtype).total for _, k in vs]
    if out is None:
        out = torch.empty(V * B * S, H, dtype=x.dtype, device=x.device)
    elif out.shape != (V * B * S, H) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("out must be a contiguous [V*B*S, H] tensor of the activations' dtype")
    if not V:
        return out, nbytes
    if x.is_cuda:
        if x.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("GPU boundary codec expects bf16 or fp32 activations")
        _fork_gpu(x.contiguous(), spec, B, S, [(0 if src is None else src, k) for src, k in vs], list(importances), out)
    else:
        for v, (src, k) in enumerate(vs):
            out[v * B * S:(v + 1) * B * S] = fake_quant(x, spec, B, S, k=k,
                                                        importance=None if src is None else importances[src])[0]
    return out, nbytes

