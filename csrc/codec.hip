// Boundary codec kernels: importance-ranked token selection and the
// quantize/pack / unpack/dequantize of the hidden state that crosses a pipeline-stage boundary.
//
// Wire message (offsets computed on the host, codec/wire.py, every section 16-byte aligned):
//   fixed k     : [header 32 B][class bitmask B x MW u32][scales][hi-class rows][lo-class rows]
//   variable k  : [header 32 B][class bitmask][k per window, B x i32][scales][lo-class rows][hi-class rows]
// (variable k = top-rho selection: each window quantizes the tokens outside its smallest importance mass
// reaching a threshold; window b's rows follow the sum of the k (or S - k) of the windows before it, and the hi
// section starts right after the Sum k lo rows, so the message is compact; the buffer has capacity for any k).
// A token whose bit is set belongs to the low-precision ("lo") class.  Rows of each class are stored in
// token order; a row's slot is the popcount of the mask bits before it, so the receiver needs nothing
// but the mask.  Row formats: 0 bf16, 1 int8, 2 int4 (two's-complement nibbles, even element in the low
// nibble), 3 int2 (ternary, 4 per byte), 9 fp16, 10 scaled fp16 (16-bit wires, below).
// Scale modes: 0 per token (fp32 [B*S]), 1 per window for the
// lo class (fp32 [B], reference Q1 "one global max-abs" int4), 2 per channel (fp32 [B*H]; reference
// channel_8/4/1_max store max|x_c|, channel_1_mean stores mean_c + 1e-8), 3 none (pass-through).
// Activations are bf16 or fp32 (the fp32 execution mode); row format 4 keeps a row in fp32 (the reference leaves
// its un-selected tokens in fp32, Experiments/Qwen2-0.5B/qwen_layer_wise.py:54-70).
#include "common.h"
#include <utility>

enum { FMT_BF16 = 0, FMT_INT8 = 1, FMT_INT4 = 2, FMT_INT2 = 3, FMT_F32 = 4, FMT_MXFP4 = 5, FMT_MXFP8 = 6, FMT_GRP = 7,
       FMT_GRPR = 8, FMT_F16 = 9, FMT_F16S = 10, FMT_MXFP6 = 11, FMT_MXBF6 = 12,
       FMT_MXFP4R = 13, FMT_MXFP8R = 14, FMT_MXFP6R = 15, FMT_MXBF6R = 16,
       FMT_INT8O = 17, FMT_INT4O = 18, FMT_INT2O = 19,
       FMT_INT8R = 20, FMT_INT4R = 21, FMT_INT2R = 22,
       FMT_INT8F = 23, FMT_INT4F = 24, FMT_INT2F = 25, FMT_NVFP4 = 26 };
// Outlier rows (FMT_INT8O / FMT_INT4O / FMT_INT2O; codec/wire.py with_outliers resolves the int classes of a per-token
// codec to them): [the plain twin's code bytes][8 fp32 values][8 uint16 channels], the twin's bytes + OUT_TAIL.  The 8
// channels with the largest abs_bits(x) (NaN > Inf > finite; ties to the lower channel), listed in that order, cross
// with their exact bits; the row's scale (in the message's scale section, as for the twin) is tok_scale of the max|x|
// of the OTHER channels and the codes are tok_code of the row with the 8 replaced by +0.  Decode: the twin's
// tok_value, then pair r = 0 .. 7 overwrites its channel; a channel >= H in a received row decodes the row to NaN.
// The code sections are multiples of 8 bytes (H % 32 == 0), so the tail is 4-byte aligned and every access to it is 4
// or 2 bytes wide.  Messages with such rows run the OUT instantiations of pack_kernel / unpack_kernel (every such
// branch under `if constexpr (OUT)`; SC_TOKEN only, not next to head-group, 16-bit, 6-bit or rotated rows), so the
// instantiations every other codec runs keep their instruction stream.  Header word 7 is hi_fmt | lo_fmt << 8 and
// unpack_kernel<OUT> decodes a message that says otherwise to NaN.  The selection: out_extract, the patch: out_patch.
enum { OUT_K = 8, OUT_TAIL = 6 * OUT_K };
__device__ __forceinline__ bool is_out_fmt(int fmt) { return fmt >= FMT_INT8O && fmt <= FMT_INT2O; }
template <bool OUT>
__device__ __forceinline__ int out_twin(int fmt) {   // an outlier row's plain twin, any other format itself
  if constexpr (OUT) {
    if (is_out_fmt(fmt)) return fmt - (FMT_INT8O - FMT_INT8);
  }
  return fmt;
}
// Rotated per-token int rows (FMT_INT8R / FMT_INT4R / FMT_INT2R; codec/wire.py with_row_rot resolves the int classes of
// a per-token codec to them): the bytes of the plain twin - its codes, the scale in the message's scale section - but
// codes and scale describe y = H128 x / 8 of every 128-channel block, H128 the natural-order Sylvester matrix: one
// massive channel is spread over its block, whose max|y| - and with it the row's one step - falls by up to 8 (QuaRot /
// SpinQuant, block-diagonal: 896 = 7 * 128).  Encode: seven fp32 butterfly stages (a, b) -> (a + b, a - b) at channel
// strides 1, 2, 4, 8, 16, 32, 64 in that order, the lower index keeping the sum, one multiply by 0.125f, then the plain
// row's path unchanged (max-abs on bit patterns, tok_scale, tok_inv, tok_code).  Decode: the integer codes as floats,
// the same seven stages (|sum| <= 128 * 127: exact), one multiply by s * 0.0625f (H128 H128 = 128 I = 8 * 16 I).  No add
// follows a multiply on either side, so there is nothing for fp contraction to fuse and the CPU oracle (codec/wire.py
// _wht128) agrees bit for bit.  The unit is the token row: a NaN / Inf in any block, or a finite row whose butterflies
// overflow (max-abs from about 2^120 up), makes y - so the row's scale, so the whole decoded row - non-finite: loud,
// never clipped.  Where the stages run: wht_row16.  Messages with such rows run the RR instantiations of pack_kernel /
// unpack_kernel (every rotated branch under `if constexpr (RR)`; SC_TOKEN and H % 128 == 0 only, not next to
// head-group, 16-bit, 6-bit, rotated MX or outlier rows), so the instantiations every other codec runs keep their
// instruction stream.  Header word 7 is hi_fmt | lo_fmt << 8 and unpack_kernel<RR> decodes a message that says
// otherwise to NaN.
__device__ __forceinline__ bool is_rr_fmt(int fmt) { return fmt >= FMT_INT8R && fmt <= FMT_INT2R; }
template <bool RR>
__device__ __forceinline__ int rr_twin(int fmt) {   // a rotated int row's plain twin, any other format itself
  if constexpr (RR) {
    if (is_rr_fmt(fmt)) return fmt - (FMT_INT8R - FMT_INT8);
  }
  return fmt;
}
// Row-rotated per-token int rows (FMT_INT8F / FMT_INT4F / FMT_INT2F; with_row_rot "full"): the plain twin's bytes again,
// but codes and scale describe y = e H x of the whole row - one massive channel is spread over all H channels, so the
// row's max|y| falls by up to sqrt(H), not sqrt(128).  H = 2^n (n = 7 .. 12): the natural-order Sylvester matrix, stages
// at strides 1 .. 2^(n-1), e = 2^-floor(n/2), decode factor s 2^-ceil(n/2) - at H = 128 the h128 row.  H = 28 2^m (m = 5,
// 6, 7: 896, 1792, 3584; channel a 2^m + b): H = H28 (x) H_2^m with H28 the Paley type II matrix of make_h28.  Encode: the
// m Sylvester stages along b, the 28-point stage out[a'] = sum_a H28[a'][a] t[a] in ascending a from +-t[0] (h28_dot:
// the order is part of the format - it is what makes non-integer rows byte-identical to the CPU's), one multiply by
// e = 2^-(2 + floor(m/2)).  Decode: the codes as floats, the 28-point stage (H28 is symmetric; |sum| <= 3584 * 127:
// exact), the m stages, one multiply by s d with d = fp32(1/28) 2^(2 + floor(m/2) - m), s d rounded once.  No add follows
// a multiply.  The unit is the token row; a finite row overflows from a max-abs of about 2^(127 - log2 H).  Where it
// runs: rot_full_row, in the RF instantiations of pack_kernel / unpack_kernel under the RR instantiations' rules
// (SC_TOKEN only; not next to head-group, 16-bit, 6-bit, rotated MX, outlier or h128 rows; header word 7 names both
// formats).
__device__ __forceinline__ bool is_rf_fmt(int fmt) { return fmt >= FMT_INT8F && fmt <= FMT_INT2F; }
template <bool RF>
__device__ __forceinline__ int rf_twin(int fmt) {   // a row-rotated int row's plain twin, any other format itself
  if constexpr (RF) {
    if (is_rf_fmt(fmt)) return fmt - (FMT_INT8F - FMT_INT8);
  }
  return fmt;
}
constexpr bool rf_size_ok(int H) {   // 2^7 .. 2^12, or 28 * 2^m for m = 5, 6, 7
  return (H >= 128 && H <= 4096 && !(H & (H - 1))) || H == 896 || H == 1792 || H == 3584;
}
// 16-bit wire formats of the rows a codec keeps in the activation dtype (codec/wire.py with_native_wire: the NATIVE
// class of a codec resolves to one of them instead of the activation dtype, so fp32 activations cross at 2 B per
// element).  FMT_BF16 (above): round to nearest even.  FMT_F16: IEEE binary16, the fp32 value converted with round to
// nearest even (the compiler's conversion, never a round-toward-zero pack); subnormals and -0 are kept; a finite value
// that rounds past 65504 encodes as +-Inf and decodes non-finite - loud; FMT_F16S or FMT_BF16 is the choice for
// unbounded data.  FMT_F16S (scaled fp16, self-scaled): row = [H binary16 codes][one fp32 p], 2 H + 4 bytes, so rows
// are only 4-byte aligned and every access to them is 4 bytes wide.  With a the row's max|x| (on bit patterns, NaN
// propagates): a NaN / Inf -> p = a itself (the codes are don't-care, every channel decodes non-finite); a = 0 ->
// p = 1; else p = 2^k, k = clamp(E - 141, -112, 113) with E the biased exponent field of a (0 for a denormal;
// E - 141 = E - 127 - 14).  p and inv = 2^-k are built from integer bit patterns, both normal floats.  Code of channel
// c: fp16_rne(x_c * inv); decode: float(code_c) * p - one fp32 multiply each, no add after a multiply anywhere, so
// nothing for fp contraction to fuse.  With k unclamped a * inv is in [2^14, 2^15): no finite row overflows fp16, and
// |x' - x| <= max(2^-11 |x|, 2^(k - 25)); only a value within half an fp16 ulp of 2^128 (a >= 2^128 - 2^116, the
// fp32 maximum included) decodes to Inf, as it does in bf16.  Below a = 2^-98 the lower clamp holds k at -112: finite
// and bounded, not accurate.  Messages with FMT_F16 / FMT_F16S rows run the W16 instantiations of pack_kernel /
// unpack_kernel (every such branch under `if constexpr (W16)`), so the instantiations every other codec runs keep
// their instruction stream; no native-hi codec has head-group lo rows, so ROT x W16 is rejected (run_codec).
// Head-group rows (FMT_GRP): every 64-channel group g (one head's width) has its own bit width b_g in {2, 3, 4, 5, 6, 8}
// (the plan: one byte per group in the message at off_plan, chosen from the boundary's channel-group sensitivity) and
// its own max-abs scale s = max|x| / qmax_b (qmax = 2^(b-1) - 1: 1 / 3 / 7 / 15 / 31 / 127): row = [group 0 codes
// (8 b_0 bytes)] ... [group G-1 codes][G fp32 scales]; the group's 64 two's-complement b-bit codes form one
// little-endian bit stream (code c at bits [b c, b c + b)), so 8 consecutive codes are b whole bytes.
// Rotated head-group rows (FMT_GRPR): the bytes of FMT_GRP rows (same plan, same row size), but the codes and the scale
// of a group describe y = H64 x / 8 with H64 the 64 x 64 Sylvester / Walsh-Hadamard +-1 matrix (H64 / 8 orthonormal and
// symmetric, so its own inverse; QuaRot / SpinQuant): a massive channel's energy spreads over its group, max|y| - and
// with it the step - falls by up to 8.  Encode: butterflies (a, b) -> (a + b, a - b) in fp32 at channel strides 1, 2,
// 4, 8, 16, 32 in that order, times 0.125f (exact), then exactly FMT_GRP's quantizer.  Decode: the same butterflies
// on the integer codes (exact, |sum| <= 64 * 127), then x' = float(sum) * (s * 0.125f) - one rounding per factor, no
// add after a multiply anywhere, so nothing for fp contraction to fuse and the CPU oracle (codec/wire.py) agrees bit
// for bit.  Messages with rows of this format run the ROT instantiations of pack_kernel / unpack_kernel
// (pack_kernel<NCH, T, true>, every rotated branch under `if constexpr (ROT)`), so the instantiations every other
// codec runs keep their instruction stream.
// One definition each, shared by pack_kernel and unpack_kernel: row_slot<ROT> (a row's class, format, qmax, window and
// message address: the fixed-k / variable-k addressing), SELF_SCALED (the formats with no entry in the scale
// section), grp_walk (a group's stream offset and width from the message's plan bytes, and whether they are usable).
// OCP microscaling rows (FMT_MXFP4: E2M1 codes, FMT_MXFP8: E4M3 codes): blocks of 32 consecutive channels share one
// E8M0 scale 2^(floor(log2 max|x|) - emax) (emax 2 / 8), stored after the row's codes: [codes][H/32 scale bytes].
// Quantize / dequantize with gfx950's scaled converts (v_cvt_scalef32_pk_fp4_f32 / _fp8_f32 and the inverses:
// round-to-nearest-even of x / scale, saturating).
// MXFP6 rows (FMT_MXFP6: E2M3 codes, bias 1, max 7.5, emax 2; FMT_MXBF6: E3M2 codes, bias 3, max 28, emax 4; no Inf /
// NaN codes, subnormals kept; codec/wire.py with_mx_elem resolves a codec's FMT_MXFP4 classes to one of them): the MX
// row layout [codes][H/32 E8M0 bytes] with a block's 32 six-bit codes as one little-endian bit stream of 24 bytes, code
// c at bits [6 c, 6 c + 6), sign in the code's top bit; 25 H / 32 bytes a row (4-byte aligned when H % 128 == 0, as
// at H = 896: 700 bytes), and every access to a row is 4 bytes wide (or one byte, for the scales).  Scale byte:
// mx_scale_byte, as for the other MX rows.
// Code: round to nearest even of clamp(x / X, +-max) on the element grid - the clamp first (x / X reaches (7.5, 8) /
// (28, 32)), in software: nothing depends on whether the convert saturates.  gfx950's fp6 converts take a whole block
// per lane (v_cvt_scalef32_2xpk16_{fp6,bf6}_f32: 2 x 16 floats -> 6 dwords; v_cvt_scalef32_pk32_f32_{fp6,bf6} back), so
// these rows have their own data movement (mx6_pack_row / mx6_unpack_row: the row goes through the wave's LDS slice
// from the 8-channels-per-lane layout of every other format to one block per lane).  The encode's result interleaves
// its operands - code 2 p is operand 0's element p, code 2 p + 1 operand 1's (measured: tools/probes/mx6probe.hip; the
// HIP headers' fallback concatenates them instead) - so operand 0 gets the block's even channels and operand 1 the odd
// ones and the six dwords are the wire's stream; the decode returns element c from bits [6 c, 6 c + 6).  Messages with
// such rows run the MX6 instantiations of pack_kernel / unpack_kernel (every 6-bit branch under `if constexpr (MX6)`;
// they handle every other format but FMT_GRPR, FMT_F16 and FMT_F16S, which run_codec rejects next to 6-bit rows), so
// the instantiations every other codec runs keep their instruction stream and allocate no LDS.  Header word 7 of such
// a message is hi_fmt | lo_fmt << 8; unpack_kernel<MX6> decodes every row of a message that says otherwise to NaN.
// Rotated MX rows (FMT_MXFP4R / FMT_MXFP8R / FMT_MXFP6R / FMT_MXBF6R; codec/wire.py with_mx_rot resolves every MX class
// of a codec to its twin): the bytes of the plain row, [codes][H/32 E8M0 bytes], but codes and scale byte describe
// y = H32 x / 4 of the block, H32 the natural-order Sylvester matrix (y_i = sum_j (-1)^popcount(i & j) x_j): a loud
// channel of a block is spread over its 32 channels, and E2M1 no longer flushes what lies below 1/12 of it.  Encode:
// five fp32 butterfly stages (a, b) -> (a + b, a - b) at channel strides 1, 2, 4, 8, 16 in that order, the lower index
// keeping the sum, then one multiply by 0.25f, then the plain row's quantizer on y (max-abs on bit patterns,
// mx_scale_byte, software clamp, convert).  Decode: the plain row's values y' = X grid, the same five stages, one
// multiply by 0.125f (H32 H32 = 32 I; 32 / (4 * 8) = 1).  No multiply precedes an add anywhere, so there is nothing for
// fp contraction to fuse and the CPU oracle (codec/wire.py _wht32) agrees bit for bit; the decoder's sums are
// multiples of the grid quantum bounded by 32 max (9 / 11 / 14 / 23 bits for E2M1 / E2M3 / E3M2 / E4M3): exact, only
// the ends of the exponent range round.  A block holding a NaN / Inf rotates to non-finite y: byte 255, 32 NaNs.  So
// does a finite block whose butterflies overflow (max-abs from about 2^123 up) - loud, never clipped.
// Where the stages run: a 4- or 8-bit row keeps the 8-channels-per-lane layout, so a block is the 4 lanes of one quad -
// strides 1, 2, 4 are wht8 on a lane's own values, strides 8 and 16 pair lanes ^1 and ^2 of the quad by DPP quad_perm
// moves (wht_quad: 16 per lane and chunk, on the VALU's own operand path - a constant __shfl_xor compiles to
// ds_bpermute_b32 through the LDS crossbar, what FMT_GRPR's wht_lanes pays for).  A 6-bit row has the whole block on
// one lane after mx6_pack_row's transposition (before mx6_unpack_row's): all five stages are wht32 on its 32 values,
// 80 add / sub, on the natural-order block - before the even / odd operand interleave of the convert.  Messages with
// such rows run the MXR instantiations of pack_kernel / unpack_kernel (every rotated branch under `if constexpr
// (MXR)`; MXR x MX6 when a class is 6-bit, the only ones of the MXR family with LDS), so the instantiations every
// other codec runs keep their instruction stream.  Header word 7 is hi_fmt | lo_fmt << 8 as for 6-bit rows, and
// unpack_kernel<MXR> decodes a message that says otherwise to NaN.  Not next to FMT_GRPR, FMT_F16, FMT_F16S rows.
// NVFP4 rows (FMT_NVFP4; codec/wire.py with_mx_elem "nvfp4" resolves a codec's FMT_MXFP4 classes to it): E2M1 codes in
// blocks of 16 consecutive channels, each with an E4M3 scale byte (OCP e4m3fn, bias 7, subnormals kept), and one fp32
// second-level scale g a row: [H/2 code bytes][H/16 scale bytes][g], 9 H / 16 + 4 bytes, byte-aligned only (H = 32: 22) -
// the code dwords and g are written and read at any address, as MXFP4 rows' dwords are.  Encode, every step one fp32
// operation rounded once, `/` the correctly rounded quotient: g = am / 2688 with am the row's max-abs on bit patterns
// (2688 = 448 * 6: the loudest block's scale is the E4M3 maximum; a NaN / Inf in the row makes g non-finite); per block
// w = (amb / g) / 6 with amb the block's max-abs, sb = the E4M3 round-to-nearest-even byte of min(w, 448) - the clamp
// first, the convert does not saturate and (am / g) / 6 can round above 448; g == 0 (an all-zero row) -> sb = 0;
// d = e4m3(sb) * g; sb == 0 or d < 2^-126 (zero or denormal) -> the block's codes are 0, else code = E2M1 round to
// nearest, ties to the even code, of clamp(x / d, +-6), the sign kept on what rounds to zero.  Decode: d the same,
// value = e2m1(code) * d.  No add follows a multiply, so there is nothing for fp contraction to fuse and the CPU oracle
// (codec/wire.py _nv_pack / _nv_unpack) agrees bit for bit.  The unit of the non-finite rule is the token row: a
// non-finite g decodes the whole row to NaN (only such a row's code and scale bytes may differ from the CPU's); a NaN w
// takes the clamp's 448, so the encoder never writes the E4M3 NaN bytes 0x7F / 0xFF - a received one makes d, and with
// it the block's 16 channels, NaN.  The E2M1 and E4M3 converts run with scale operand 1.0f (a power of two, as every
// scale operand in this file: what the hardware does with that operand's mantissa bits is not relied on); x / d and
// code * d are VALU operations.  Where it runs: nv_pack8 / nv_unpack8, in the NV4 instantiations of pack_kernel /
// unpack_kernel (every such branch under `if constexpr (NV4)`; beside native and plain FMT_MXFP8 rows, not next to
// head-group, 16-bit, 6-bit, rotated MX, outlier or rotated int rows), so the instantiations every other codec runs
// keep their instruction stream.  Header word 7 is hi_fmt | lo_fmt << 8 and unpack_kernel<NV4> decodes a message that
// says otherwise to NaN.
enum { SC_TOKEN = 0, SC_WINDOW = 1, SC_CHANNEL = 2, SC_NONE = 3 };
enum { CH_MAXABS = 0, CH_MEAN = 1 };

struct CodecArgs {
  void* x; uint8_t* msg;
  long long off_mask, off_scale, off_hi, off_lo;
  long long off_kvec;           // >= 0: variable-k layout (k per window at msg + off_kvec), else fixed k
  long long off_plan;           // >= 0: FMT_GRP bit plan (one byte per 64-channel group)
  int B, S, H, k, mw;           // mw: mask words per window
  int hi_fmt, lo_fmt, scale_mode, qmax_hi, qmax_lo, ch_kind;
  int grp_code_bytes;           // FMT_GRP / FMT_GRPR: sum over groups of 8 b_g (row = codes + 4 G scale bytes)
};

template <bool W16, bool MX6, bool MXR = false, bool OUT = false, bool RR = false, bool RF = false, bool NV4 = false>
__device__ __forceinline__ int fmt_row_bytes(int fmt, int H) {
  if constexpr (NV4) {   // E2M1 codes, one E4M3 scale byte per 16 channels, the row's fp32 g
    if (fmt == FMT_NVFP4) return 9 * (H / 16) + 4;
  }
  if constexpr (RF) {    // a row-rotated int row has the bytes of its plain twin
    if (is_rf_fmt(fmt)) return fmt == FMT_INT8F ? H : fmt == FMT_INT4F ? H / 2 : H / 4;
  }
  if constexpr (RR) {    // a rotated int row has the bytes of its plain twin
    if (is_rr_fmt(fmt)) return fmt == FMT_INT8R ? H : fmt == FMT_INT4R ? H / 2 : H / 4;
  }
  if constexpr (OUT) {   // an outlier row has the bytes of its plain twin and the tail
    if (is_out_fmt(fmt)) return (fmt == FMT_INT8O ? H : fmt == FMT_INT4O ? H / 2 : H / 4) + OUT_TAIL;
  }
  if constexpr (W16) {
    if (fmt == FMT_F16) return 2 * H;
    if (fmt == FMT_F16S) return 2 * H + 4;
  }
  if constexpr (MX6) {
    if (fmt == FMT_MXFP6 || fmt == FMT_MXBF6) return 25 * (H / 32);
  }
  if constexpr (MXR) {   // a rotated row has the bytes of its plain twin
    if (fmt == FMT_MXFP4R) return H / 2 + H / 32;
    if (fmt == FMT_MXFP8R) return H + H / 32;
    if constexpr (MX6) {
      if (fmt == FMT_MXFP6R || fmt == FMT_MXBF6R) return 25 * (H / 32);
    }
  }
  return fmt == FMT_F32 ? 4 * H : fmt == FMT_BF16 ? 2 * H : fmt == FMT_INT8 ? H : fmt == FMT_INT4 ? H / 2 :
         fmt == FMT_MXFP4 ? H / 2 + H / 32 : fmt == FMT_MXFP8 ? H + H / 32 : H / 4;
}
template <bool ROT, bool W16, bool MX6, bool MXR = false, bool OUT = false, bool RR = false, bool RF = false,
          bool NV4 = false>
__device__ __forceinline__ int row_bytes(const CodecArgs& a, int fmt) {
  if constexpr (ROT) {
    if (fmt == FMT_GRPR) return a.grp_code_bytes + 4 * (a.H / 64);
  }
  return fmt == FMT_GRP ? a.grp_code_bytes + 4 * (a.H / 64) : fmt_row_bytes<W16, MX6, MXR, OUT, RR, RF, NV4>(fmt, a.H);
}
// Formats whose rows carry their own scales (or none): no entry in the message's scale section.  A macro, and the
// rotated format joined with `|`: the compiler simplifies the body of an inlined function on its own first, and the
// rotated pack instantiations then allocate 66 / 82 instead of 56 / 74 VGPRs (NCH 2 / 4: a wave per SIMD less).
#define SELF_SCALED(ROT, W16, MX6, MXR, NV4, fmt) \
  (((fmt) == FMT_BF16 || (fmt) == FMT_F32 || (fmt) == FMT_MXFP4 || (fmt) == FMT_MXFP8 || (fmt) == FMT_GRP) | \
   ((ROT) && (fmt) == FMT_GRPR) | ((W16) && ((fmt) == FMT_F16 || (fmt) == FMT_F16S)) | \
   ((MX6) && ((fmt) == FMT_MXFP6 || (fmt) == FMT_MXBF6)) | \
   ((MXR) && ((fmt) == FMT_MXFP4R || (fmt) == FMT_MXFP8R || (fmt) == FMT_MXFP6R || (fmt) == FMT_MXBF6R)) | \
   ((NV4) && (fmt) == FMT_NVFP4))

// Max-abs reductions of the codec propagate NaN (a unit holding a NaN / Inf must decode non-finite, and fmaxf drops a
// NaN operand): they run on the bit pattern of |x| as an unsigned integer.  For non-negative floats the integer order
// is the float order (denormals included), Inf is above every finite value and every NaN above Inf - the max of a
// unit with a NaN is a NaN, with an Inf and no NaN Inf, and for finite values the very float fmaxf returns.
// (wave_max / block_max of common.h keep fmaxf: their other users want it.)
__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t umax8(const float (&v)[8]) {   // bits of max|v|
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) m = umax(m, abs_bits(v[e]));
  return m;
}
__device__ __forceinline__ void fill8(float (&o)[8], float x) {
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = x;
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umax(v, __shfl_xor(v, o, 64));
  return v;
}
template <int NT>
__device__ __forceinline__ uint32_t block_umax(uint32_t v, uint32_t* red) {
  v = wave_umax(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) red[w] = v;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) t = umax(t, red[i]);
  __syncthreads();
  return t;
}

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// number of lo-class tokens before token j in window b, and the class of j
__device__ __forceinline__ int lo_prefix(const uint32_t* __restrict__ mask, int mw, int j, bool& is_lo) {
  const int lane = threadIdx.x & 63;
  const int wj = j >> 5;
  int cnt = 0;
  for (int w = lane; w < wj; w += 64) cnt += __popc(mask[w]);
  cnt = wave_isum(cnt);
  const uint32_t word = mask[wj];
  is_lo = (word >> (j & 31)) & 1u;
  return cnt + __popc(word & ((1u << (j & 31)) - 1u));
}

// ---------------------------------------------------------------------------------------------
// Token selection: one workgroup per window sorts the window's (importance, position) pairs
// ascending with an LDS bitonic sort of 64-bit keys (order-preserving float bits << 32 | position: ties by
// position, NaN ranked above +inf, -0 == +0 - the order of a stable torch.sort) and marks the first k positions
// as the lo class.
//   mode 0 (ratio)  : k given (reference int(ratio * S), qwen_layer_wise.py:57).
//   mode 1 (top-rho): in descending order, keep the shortest prefix whose mass reaches thr = 1 - 0.1 ratio and
//                     quantize the rest: keep = first i with sum_{j<i} desc_j >= thr (thr <= 0 -> 0, none -> S),
//                     k = S - keep (the intended semantics of pythia_model.py:92-112, its token-id indexing bug
//                     B21 fixed); the exclusive prefix sums are an LDS block scan.  k is written to kvec[b].
__device__ __forceinline__ uint32_t ord_key(float f) {
  if (f != f) return 0xFFFFFFFFu;                  // NaN last
  uint32_t u = __float_as_uint(f == 0.f ? 0.f : f);  // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_val(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

constexpr int SEL_T = 512;
// A window's sort key (shared by select_sort_kernel and rank_scan_kernel) and the ascending LDS bitonic sort of P keys
// (P a power of two, the keys written and the workgroup synchronised before the call; synchronised on return).
__device__ __forceinline__ unsigned long long sel_key(float imp, int i) {
  return ((unsigned long long)ord_key(imp) << 32) | (unsigned)i;
}
__device__ __forceinline__ void bitonic_sort_keys(unsigned long long* keys, int P) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += SEL_T) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keys[i], c = keys[ixj];
          if (((i & k) == 0) == (a > c)) { keys[i] = c; keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
}
__global__ __launch_bounds__(SEL_T) void select_sort_kernel(const float* __restrict__ imp, int S, int P, int mode,
                                                            int k_fixed, float thr, uint32_t* __restrict__ mask_out,
                                                            int mw, int* __restrict__ kvec) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];  // P keys, then mw mask words
  uint32_t* mwords = (uint32_t*)(keys + P);
  __shared__ float part[SEL_T];
  __shared__ int cut;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* ib = imp + (size_t)b * S;
  for (int i = tid; i < P; i += SEL_T)
    keys[i] = i < S ? sel_key(ib[i], i) : ~0ull;
  for (int w = tid; w < mw; w += SEL_T) mwords[w] = 0u;
  if (tid == 0) cut = S;
  __syncthreads();
  bitonic_sort_keys(keys, P);
  int kk = k_fixed;
  if (mode == 1) {
    // descending value i = keys[S-1-i]; thread t owns the contiguous run [t*C, t*C + C) of descending positions
    const int C = (S + SEL_T - 1) / SEL_T;
    const int i0 = tid * C;
    float run = 0.f;
    for (int e = 0; e < C && i0 + e < S; ++e) run += key_val((uint32_t)(keys[S - 1 - (i0 + e)] >> 32));
    part[tid] = run;
    __syncthreads();
    for (int off = 1; off < SEL_T; off <<= 1) {  // Hillis-Steele inclusive scan of the run sums
      const float v = tid >= off ? part[tid - off] : 0.f;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    float excl = tid ? part[tid - 1] : 0.f;
    for (int e = 0; e < C && i0 + e < S; ++e) {
      if (excl >= thr) { atomicMin(&cut, i0 + e); break; }
      excl += key_val((uint32_t)(keys[S - 1 - (i0 + e)] >> 32));
    }
    __syncthreads();
    kk = S - cut;
  }
  for (int p = tid; p < kk; p += SEL_T) {
    const int idx = (int)(keys[p] & 0xFFFFFFFFu);
    atomicOr(&mwords[idx >> 5], 1u << (idx & 31));
  }
  __syncthreads();
  uint32_t* mb = mask_out + (size_t)b * mw;
  for (int w = tid; w < mw; w += SEL_T) mb[w] = mwords[w];
  if (kvec && tid == 0) kvec[b] = kk;
}

// Variable-k layout: lo rows of the windows before b (Kb) and in total (Kt), by one wave.
__device__ __forceinline__ void kvar_prefix(const CodecArgs& a, int b, int& Kb, int& Kt) {
  const int lane = threadIdx.x & 63;
  const int* kv = (const int*)(a.msg + a.off_kvec);
  int before = 0, all = 0;
  for (int w = lane; w < a.B; w += 64) {
    const int v = kv[w];
    all += v;
    before += w < b ? v : 0;
  }
  Kb = wave_isum(before);
  Kt = wave_isum(all);
}

// Where row `row` (token j of window b) lives in the message and how it is coded: its class from the mask, its slot
// among the class's rows of its window (lo_prefix), the class's rows of the windows before (b k / b (S - k) for fixed
// k, the k vector's prefix sum for variable k, whose hi section starts right after the Sum k lo rows).
struct RowSlot { uint8_t* p; int fmt, qmax, b; };
template <bool ROT, bool W16, bool MX6, bool MXR = false, bool OUT = false, bool RR = false, bool RF = false,
          bool NV4 = false>
__device__ __forceinline__ RowSlot row_slot(const CodecArgs& a, int row) {
  const int b = row / a.S, j = row - b * a.S;
  const uint32_t* mask = (const uint32_t*)(a.msg + a.off_mask) + (size_t)b * a.mw;
  bool is_lo;
  const int slot_lo = lo_prefix(mask, a.mw, j, is_lo);
  const int fmt = is_lo ? a.lo_fmt : a.hi_fmt;
  const int rb = row_bytes<ROT, W16, MX6, MXR, OUT, RR, RF, NV4>(a, fmt);
  uint8_t* p;
  if (a.off_kvec >= 0) {
    int Kb, Kt;
    kvar_prefix(a, b, Kb, Kt);
    const long long off_hi =
        a.off_lo + (((long long)Kt * row_bytes<ROT, W16, MX6, MXR, OUT, RR, RF, NV4>(a, a.lo_fmt) + 15) & ~15ll);
    p = is_lo ? a.msg + a.off_lo + ((size_t)Kb + slot_lo) * rb
              : a.msg + off_hi + ((size_t)b * a.S - Kb + (j - slot_lo)) * rb;
  } else {
    p = is_lo ? a.msg + a.off_lo + ((size_t)b * a.k + slot_lo) * rb
              : a.msg + a.off_hi + ((size_t)b * (a.S - a.k) + (j - slot_lo)) * rb;
  }
  return {p, fmt, is_lo ? a.qmax_lo : a.qmax_hi, b};
}

// Per-(window, channel) statistics over the window's rows (optionally only lo-class rows).
// mode 0: max|x|, mode 1: mean(x) + 1e-8.   grid (B, ceil(H/64)), 256 threads = 4 row groups x 64 ch.
__device__ __forceinline__ float ldx(const bf16_t* p, size_t i) { return bf2f(p[i]); }
__device__ __forceinline__ float ldx(const float* p, size_t i) { return p[i]; }

template <class T>
__global__ __launch_bounds__(256) void channel_stats_kernel(const T* __restrict__ x,
                                                            const uint32_t* __restrict__ mask, int mask_stride,
                                                            float* __restrict__ out, int S, int H, int mode,
                                                            int only_lo) {
  __shared__ float red[4][64];
  const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const uint32_t* mb = mask + (size_t)b * mask_stride;
  float acc = 0.f;
  uint32_t am = 0;   // mode 0: bits of the running max|x| (NaN-propagating, see abs_bits)
  if (c < H) {
    for (int j = rg; j < S; j += 4) {
      if (only_lo && !((mb[j >> 5] >> (j & 31)) & 1u)) continue;
      const float xv = ldx(x, ((size_t)b * S + j) * H + c);
      if (mode == 0) am = umax(am, abs_bits(xv));
      else acc += xv;
    }
  }
  red[rg][threadIdx.x & 63] = mode == 0 ? __uint_as_float(am) : acc;
  __syncthreads();
  if (rg == 0 && c < H) {
    const int l = threadIdx.x;
    float r = mode == 0 ? __uint_as_float(umax(umax(__float_as_uint(red[0][l]), __float_as_uint(red[1][l])),
                                               umax(__float_as_uint(red[2][l]), __float_as_uint(red[3][l]))))
                        : (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    out[(size_t)b * H + c] = mode == 0 ? r : r / (float)S + 1e-8f;
  }
}

// Row max of max-abs values (channel_stats mode 0: non-negative or NaN), NaN-propagating.
__global__ __launch_bounds__(256) void rowmax_kernel(const float* __restrict__ in, float* __restrict__ out, int H) {
  __shared__ uint32_t red[4];
  const float* r = in + (size_t)blockIdx.x * H;
  uint32_t m = 0;
  for (int c = threadIdx.x; c < H; c += 256) m = umax(m, abs_bits(r[c]));
  m = block_umax<256>(m, red);
  if (threadIdx.x == 0) out[blockIdx.x] = __uint_as_float(m);
}

// ---------------------------------------------------------------------------------------------
template <int NCH>
__device__ __forceinline__ void load_row8(const float* __restrict__ src, int H, float (&v)[NCH][8]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col < H) {
      const f32x4_t a = *(const f32x4_t*)(src + col), b = *(const f32x4_t*)(src + col + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[c][e] = a[e]; v[c][4 + e] = b[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
    }
  }
}
template <int NCH>
__device__ __forceinline__ void load_row8(const bf16_t* __restrict__ src, int H, float (&v)[NCH][8]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col < H) {
      const u32x4_t w = *(const u32x4_t*)(src + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[c][2 * e] = bf_lo(w[e]); v[c][2 * e + 1] = bf_hi(w[e]); }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
    }
  }
}

__device__ __forceinline__ float qround(float t, float qmax, float qmin) { return fminf(fmaxf(rintf(t), qmin), qmax); }

// The integer rows' arithmetic in the per-token and per-window scale modes, one definition for pack_kernel,
// unpack_kernel and fork_kernel (which quantizes and dequantizes a row with no bytes in between): the per-token scale
// and its inverse from the row's max|x|, a value's code (an integer-valued float inside the format's range; the wire
// carries (int)code, so a -0 crosses as 0), and a code's value.
__device__ __forceinline__ float tok_scale(float am, int qmax) { return am / (float)qmax; }
__device__ __forceinline__ float tok_inv(float am, float s) { return am > 0.f ? 1.f / s : 0.f; }
__device__ __forceinline__ float qmin_of(int scale_mode, int qmax) {
  return scale_mode == SC_WINDOW ? -(float)(qmax + 1) : -(float)qmax;
}
__device__ __forceinline__ float tok_code(float xv, float inv, float qmaxf, float qminf) {
  return qround(xv * inv, qmaxf, qminf);
}
// reference Q1: round(clamp(x / m * 7, -8, 7))
__device__ __forceinline__ float win_code(float xv, float mul, float qmaxf, float qminf) {
  return mul > 0.f ? rintf(fminf(fmaxf(xv / mul * qmaxf, qminf), qmaxf)) : 0.f;
}
__device__ __forceinline__ float tok_value(float qf, float s) { return qf * s; }
__device__ __forceinline__ float win_value(float qf, int qmax, float s) { return qf / (float)qmax * s; }   // q / 7 * m

typedef __attribute__((ext_vector_type(2))) short s16x2_t;

// E8M0 scale byte and value of a 32-channel block (4 lanes x 8 values): 2^(floor(log2 amax) - emax); a block holding
// a NaN / Inf (amax non-finite) gets byte 255, which OCP MX defines as NaN: mx_unpack8 decodes the whole block to NaN
// (in software - nothing here depends on what the scaled converts do with an all-ones scale exponent).
enum { MX_NAN = 255 };
__device__ __forceinline__ int mx_scale_byte(float am, int emax) {
  const int ef = (int)((__float_as_uint(am) >> 23) & 0xff);
  if (ef == 255) return MX_NAN;
  const int e = am > 0.f ? ef - 127 : -127;   // denormal amax -> -127
  const int sb = e - emax + 127;
  return sb < 0 ? 0 : (sb > 254 ? 254 : sb);
}
__device__ __forceinline__ float e8m0_value(int sb) { return sb ? __uint_as_float((uint32_t)sb << 23) : __uint_as_float(0x00400000u); }

// A value of lane ^ 1 (QUAD_X1) or lane ^ 2 (QUAD_X2) of the lane's quad by one DPP quad_perm move: dpp_ctrl holds the
// source lane of quad positions 0..3, two bits each ([1, 0, 3, 2] and [2, 3, 0, 1]).  Every lane of the quad must be
// active (a disabled source lane yields the `old` operand, 0).
enum { QUAD_X1 = 0xB1, QUAD_X2 = 0x4E };
template <int CTRL>
__device__ __forceinline__ uint32_t quad_mov(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}

// QUAD (the rotated instantiations only): the block's max-abs over its 4 lanes by quad moves instead of shuffles.
template <bool QUAD = false>
__device__ __forceinline__ void mx_pack8(uint8_t* __restrict__ row, int H, int col, int fmt, const float (&v)[8]) {
  const int lane = threadIdx.x & 63;
  uint32_t amb = umax8(v);
  if constexpr (QUAD) {
    amb = umax(amb, quad_mov<QUAD_X1>(amb));
    amb = umax(amb, quad_mov<QUAD_X2>(amb));
  } else {
    amb = umax(amb, __shfl_xor(amb, 1, 64));
    amb = umax(amb, __shfl_xor(amb, 2, 64));
  }
  const int sb = mx_scale_byte(__uint_as_float(amb), fmt == FMT_MXFP4 ? 2 : 8);
  const float X = e8m0_value(sb == MX_NAN ? 127 : sb);   // the codes of a NaN block are never read
  if (fmt == FMT_MXFP4) {
    uint32_t w = 0;
    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[0], v[1], X, 0);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[2], v[3], X, 1);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[4], v[5], X, 2);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[6], v[7], X, 3);
    *(uint32_t*)(row + col / 2) = w;
    if ((lane & 3) == 0) row[H / 2 + col / 32] = (uint8_t)sb;
  } else {
    // x / X can reach 2^9 > 448 (E4M3 max): clamp first - the fp8 convert does not saturate (NaN code)
    const float lim = 448.f * X;
    float c[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = fminf(fmaxf(v[e], -lim), lim);
    s16x2_t a = {0, 0}, b = {0, 0};
    a = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(a, c[0], c[1], X, false);
    a = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(a, c[2], c[3], X, true);
    b = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(b, c[4], c[5], X, false);
    b = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(b, c[6], c[7], X, true);
    u32x2_t w;
    w[0] = (uint32_t)(uint16_t)a[0] | ((uint32_t)(uint16_t)a[1] << 16);
    w[1] = (uint32_t)(uint16_t)b[0] | ((uint32_t)(uint16_t)b[1] << 16);
    *(u32x2_t*)(row + col) = w;
    if ((lane & 3) == 0) row[H + col / 32] = (uint8_t)sb;
  }
}

__device__ __forceinline__ void put4(float (&o)[8], f32x2_t p0, f32x2_t p1, f32x2_t p2, f32x2_t p3) {
  o[0] = p0[0]; o[1] = p0[1]; o[2] = p1[0]; o[3] = p1[1]; o[4] = p2[0]; o[5] = p2[1]; o[6] = p3[0]; o[7] = p3[1];
}
__device__ __forceinline__ void mx_unpack8(const uint8_t* __restrict__ row, int H, int col, int fmt, float (&o)[8]) {
  const int sb = row[(fmt == FMT_MXFP4 ? H / 2 : H) + col / 32];
  const float X = e8m0_value(sb == MX_NAN ? 127 : sb);
  if (fmt == FMT_MXFP4) {
    const uint32_t w = *(const uint32_t*)(row + col / 2);
    f32x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, X, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, X, 1);
    f32x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, X, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, X, 3);
    put4(o, p0, p1, p2, p3);
  } else {
    const u32x2_t w = *(const u32x2_t*)(row + col);
    f32x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], X, false), p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], X, true);
    f32x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], X, false), p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], X, true);
    put4(o, p0, p1, p2, p3);
  }
  if (sb == MX_NAN) fill8(o, __builtin_nanf(""));
}

// Rotated MX rows of 4- and 8-bit codes: the unnormalised 32-point Walsh-Hadamard transform of a block held 8
// consecutive channels per lane by the 4 lanes of a quad (col = (64 c + lane) 8: block = lane >> 2 of its chunk).
// Strides 1, 2, 4 are wht8 (below) on the lane's own values; strides 8 and 16 pair lanes ^1 and ^2 (wht_quad): the lane
// with the bit clear holds a and keeps a + b, its partner holds b and keeps a - b = a + (-b) - the partner flips its
// own sign bit and both add, 8 DPP moves, 8 xors and 8 adds a stride, no LDS.
// Every lane of a quad must be at the moves: H % 32 == 0 makes the col >= H early-out drop whole quads, and a row's
// format is wave-uniform (row_slot), so the lanes of a quad take the rotated branch together or not at all.
template <class V>
__device__ __forceinline__ void wht8(V (&v)[8]);
__device__ __forceinline__ void wht_quad(float (&v)[8]) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t s1 = (lane & 1u) << 31, s2 = (lane & 2u) << 30;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t u = __float_as_uint(v[e]);
    v[e] = __uint_as_float(quad_mov<QUAD_X1>(u)) + __uint_as_float(u ^ s1);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t u = __float_as_uint(v[e]);
    v[e] = __uint_as_float(quad_mov<QUAD_X2>(u)) + __uint_as_float(u ^ s2);
  }
}
// fmt: the plain twin's (FMT_MXFP4 / FMT_MXFP8); the lane's values are rotated in place (their last use)
__device__ __forceinline__ void mx_pack8_rot(uint8_t* __restrict__ row, int H, int col, int fmt, float (&y)[8]) {
  wht8(y);
  wht_quad(y);
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] *= 0.25f;
  mx_pack8<true>(row, H, col, fmt, y);
}
// A NaN block (byte 255) leaves mx_unpack8 as 32 NaNs and the butterflies as 32 NaNs.
__device__ __forceinline__ void mx_unpack8_rot(const uint8_t* __restrict__ row, int H, int col, int fmt, float (&o)[8]) {
  mx_unpack8(row, H, col, fmt, o);
  wht8(o);
  wht_quad(o);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] *= 0.125f;
}

// NVFP4 rows: a 16-channel block is the lane pair (2 i, 2 i + 1) of a chunk (col = (64 c + lane) 8: block = lane >> 1),
// so its max-abs is one DPP quad move and a umax, and both lanes of the pair compute the block's scale byte and step
// from the same operands - identically, with no second exchange.  g, the row's second-level scale, is wave-uniform.
// Both lanes of a pair must be at the move: H % 32 == 0 makes the col >= H early-out drop whole quads, so whole lane
// pairs, and a row's format is wave-uniform (row_slot).  No LDS, no shuffle through LDS, no scratch.
// a row of 9 H / 16 + 4 (or, MXFP6 rows, 25 H / 32) bytes starts on no 4-byte boundary in general: its dword accesses are
// declared unaligned (gfx950 serves them as dword accesses all the same)
typedef uint32_t __attribute__((aligned(1))) u32_una_t;
typedef float __attribute__((aligned(1))) f32_una_t;
__device__ __forceinline__ float e4m3_value(int sb) {   // the convert with scale 1.0f; bytes 0x7F / 0xFF: NaN
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((uint32_t)sb, 1.0f, false)[0];
}
// The row's g from the bits of its max-abs, in an SGPR (the division runs once per lane all the same: there is no
// scalar one).
__device__ __forceinline__ float nv_row_scale(uint32_t amb) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(__uint_as_float(amb) / 2688.0f)));
}
struct NvBlock { int sb; float d; bool live; };   // scale byte, step d = e4m3(sb) g, and whether the block has codes
__device__ __forceinline__ NvBlock nv_block(uint32_t amb, float g) {
  const float w = (__uint_as_float(amb) / g) / 6.0f;
  const float wc = w < 448.0f ? w : 448.0f;   // a NaN w (a non-finite row; 0 / 0 of a zero row) takes 448 too
  s16x2_t p = {0, 0};
  p = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(p, wc, wc, 1.0f, false);
  const int sb = g == 0.f ? 0 : (int)((uint16_t)p[0] & 255u);
  const float d = e4m3_value(sb) * g;
  return {sb, d, sb != 0 && !(d < 1.17549435e-38f)};
}
__device__ __forceinline__ void nv_pack8(uint8_t* __restrict__ row, int H, int col, const float (&v)[8], float g) {
  const int lane = threadIdx.x & 63;
  uint32_t amb = umax8(v);
  amb = umax(amb, quad_mov<QUAD_X1>(amb));
  const NvBlock k = nv_block(amb, g);
  float q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = fminf(fmaxf(v[e] / k.d, -6.0f), 6.0f);
  uint32_t w = 0;
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, q[0], q[1], 1.0f, 0);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, q[2], q[3], 1.0f, 1);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, q[4], q[5], 1.0f, 2);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, q[6], q[7], 1.0f, 3);
  *(u32_una_t*)(row + col / 2) = k.live ? w : 0u;
  if ((lane & 1) == 0) row[H / 2 + col / 16] = (uint8_t)k.sb;
}
// g: the row's, read once (nv_load_scale); a non-finite one decodes the row to NaN whatever its bytes say
__device__ __forceinline__ float nv_load_scale(const uint8_t* __restrict__ row, int H) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(*(const f32_una_t*)(row + 9 * (H / 16)))));
}
__device__ __forceinline__ void nv_unpack8(const uint8_t* __restrict__ row, int H, int col, float g, float (&o)[8]) {
  const float d = e4m3_value(row[H / 2 + col / 16]) * g;
  const uint32_t w = *(const u32_una_t*)(row + col / 2);
  f32x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1);
  f32x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3);
  put4(o, p0, p1, p2, p3);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] *= d;
  if (!(fabsf(g) < __builtin_inff())) fill8(o, __builtin_nanf(""));
}

// Rotated per-token int rows: the unnormalised 128-point Walsh-Hadamard transform of a block held 8 consecutive
// channels per lane by the 16 lanes of one DPP row (col = (64 c + lane) 8: block = lane >> 4 of its chunk), in place.
// Strides 1, 2, 4 are wht8 on the lane's own values, strides 8 and 16 wht_quad (lanes ^1 and ^2), strides 32 and 64 pair
// lanes ^4 and ^8 by the row controls of the same DPP operand path (quad_mov is one DPP move under any control):
// lane ^ 8 is a rotation of the 16-lane row by 8 (row_ror:8), lane ^ 4 the reversal of the row's 8-lane halves
// (row_half_mirror: lane ^ 7) followed by the reversal of the quads (quad_perm [3, 2, 1, 0]: lane ^ 3).  wht_quad's sign
// convention: the lane with the stride bit set flips its own sign bit, and both add the partner's value.  Five DPP
// moves, four xors and four adds per value on top of wht8 - no LDS, no ds_bpermute_b32, no scratch.
// Every lane of a DPP row must be at the moves (a disabled source lane yields 0): H % 128 == 0 makes the col >= H
// early-out drop whole 16-lane rows, and a row's format is wave-uniform (row_slot).
enum { DPP_QUAD_REV = 0x1B, DPP_ROW_ROR8 = 0x128, DPP_ROW_HALF_MIRROR = 0x141 };
__device__ __forceinline__ void wht_row16(float (&v)[8]) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t s4 = (lane & 4u) << 29, s8 = (lane & 8u) << 28;
  wht8(v);
  wht_quad(v);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t u = __float_as_uint(v[e]);
    v[e] = __uint_as_float(quad_mov<DPP_QUAD_REV>(quad_mov<DPP_ROW_HALF_MIRROR>(u))) + __uint_as_float(u ^ s4);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t u = __float_as_uint(v[e]);
    v[e] = __uint_as_float(quad_mov<DPP_ROW_ROR8>(u)) + __uint_as_float(u ^ s8);
  }
}

// FMT_GRP: the 8 lanes holding channels [64 g, 64 g + 64) of a row (8 values each) quantize their group.
// Byte offset of group g's codes = sum_{g' < g} 8 b_g'.
__device__ __forceinline__ int grp_offset(const uint8_t* __restrict__ plan, int g) {
  int o = 0;
  for (int i = 0; i < g; ++i) o += 8 * plan[i];
  return o;
}
// The 8 codes of a lane are bytes [sub b, sub b + b) of the group's stream (sub = lane & 7), b-byte aligned: whole
// 8 / 4 / 2-byte stores for b = 8 / 4 / 2, 2-byte pieces for b = 6, single bytes for b = 3 / 5.
__device__ __forceinline__ void grp_store(uint8_t* __restrict__ dst, uint64_t w, int bits) {
  if (bits == 8) {
    *(u32x2_t*)dst = u32x2_t{(uint32_t)w, (uint32_t)(w >> 32)};
  } else if (bits == 4) {
    *(uint32_t*)dst = (uint32_t)w;
  } else if (bits == 2) {
    *(uint16_t*)dst = (uint16_t)w;
  } else if (bits == 6) {
#pragma unroll
    for (int i = 0; i < 3; ++i) ((uint16_t*)dst)[i] = (uint16_t)(w >> (16 * i));
  } else {
    for (int i = 0; i < bits; ++i) dst[i] = (uint8_t)(w >> (8 * i));
  }
}
__device__ __forceinline__ uint64_t grp_load(const uint8_t* __restrict__ src, int bits) {
  if (bits == 8) {
    const u32x2_t v = *(const u32x2_t*)src;
    return (uint64_t)v[0] | ((uint64_t)v[1] << 32);
  }
  if (bits == 4) return *(const uint32_t*)src;
  if (bits == 2) return *(const uint16_t*)src;
  uint64_t w = 0;
  if (bits == 6) {
#pragma unroll
    for (int i = 0; i < 3; ++i) w |= (uint64_t)((const uint16_t*)src)[i] << (16 * i);
  } else {
    for (int i = 0; i < bits; ++i) w |= (uint64_t)src[i] << (8 * i);
  }
  return w;
}
// The quantizer of a head group, one definition for grp_pack8 and group_quant_err_kernel: the bits of the group's
// max|v| over the 8 lanes holding it (NaN / Inf if the group holds one: s, and the decode, non-finite), the scale
// s = am / qmax with its inverse (0 for an all-zero group), and a value's code as a float.  The decoder returns
// code * s (grp_unpack8).
__device__ __forceinline__ uint32_t grp_amax_bits(const float (&v)[8]) {
  uint32_t amb = umax8(v);
  amb = umax(amb, __shfl_xor(amb, 1, 64));
  amb = umax(amb, __shfl_xor(amb, 2, 64));
  amb = umax(amb, __shfl_xor(amb, 4, 64));
  return amb;
}
struct GrpQuant { float s, inv, qf; };
__device__ __forceinline__ GrpQuant grp_quant(float am, int qmax) {
  const float s = am / (float)qmax;
  return {s, am > 0.f ? 1.f / s : 0.f, (float)qmax};
}
__device__ __forceinline__ float grp_q(float v, const GrpQuant& k) { return qround(v * k.inv, k.qf, -k.qf); }

__device__ __forceinline__ void grp_pack8(uint8_t* __restrict__ row, const CodecArgs& a, int col,
                                          const float (&v)[8]) {
  const int lane = threadIdx.x & 63;
  const uint8_t* plan = a.msg + a.off_plan;
  const int g = col >> 6, bits = plan[g];
  const GrpQuant k = grp_quant(__uint_as_float(grp_amax_bits(v)), (1 << (bits - 1)) - 1);
  const uint64_t mask = (1ull << bits) - 1;
  uint64_t w = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) w |= ((uint64_t)(int64_t)(int)grp_q(v[e], k) & mask) << (bits * e);
  const int sub = lane & 7;
  grp_store(row + grp_offset(plan, g) + sub * bits, w, bits);
  if (sub == 0) *(float*)(row + a.grp_code_bytes + 4 * g) = k.s;
}
// A group's place in a row as the MESSAGE's plan bytes give it, for the decoders: byte offset of its stream (never
// negative: unsigned), its width, and `bad`: a width outside GROUP_BITS (a corrupt or version-mismatched message) in
// this group or one before it, or a group stream reaching past the row's code bytes.  A bad group decodes to NaN -
// loud - instead of a shift by 32 or a read past the row (invalid widths count 0 bytes in the offset).
__device__ __forceinline__ bool grp_bits_ok(int b) { return b == 2 || b == 3 || b == 4 || b == 5 || b == 6 || b == 8; }
struct GrpWalk { uint32_t off; int bits; bool bad; };
__device__ __forceinline__ GrpWalk grp_walk(const CodecArgs& a, int g) {
  const uint8_t* plan = a.msg + a.off_plan;
  int off = 0;
  bool bad = false;
  for (int i = 0; i < g; ++i) {
    const int b = plan[i];
    bad |= !grp_bits_ok(b);
    off += grp_bits_ok(b) ? 8 * b : 0;
  }
  const int bits = plan[g];
  bad |= !grp_bits_ok(bits) || off + 8 * bits > a.grp_code_bytes;
  return {(uint32_t)off, bits, bad};
}
// Code e of a lane's 8: the sign-extended b-bit field at bit b e of its b bytes.
__device__ __forceinline__ int grp_code(uint64_t w, int bits, int e) {
  return ((int)((uint32_t)(w >> (bits * e)) << (32 - bits))) >> (32 - bits);
}
__device__ __forceinline__ void grp_unpack8(const uint8_t* __restrict__ row, const CodecArgs& a, int col,
                                            float (&o)[8]) {
  const int lane = threadIdx.x & 63;
  const int g = col >> 6, sub = lane & 7;
  const GrpWalk k = grp_walk(a, g);
  const int bits = k.bits;
  if (k.bad) {
    fill8(o, __builtin_nanf(""));
    return;
  }
  const uint64_t w = grp_load(row + k.off + sub * bits, bits);
  const float s = *(const float*)(row + a.grp_code_bytes + 4 * g);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (float)grp_code(w, bits, e) * s;
}

// FMT_GRPR: the unnormalised 64-point Walsh-Hadamard transform of a group held 8 consecutive channels per lane by the
// 8 lanes sharing lane >> 3.  Channel strides 1, 2, 4 pair values of one lane (wht8), strides 8, 16, 32 pair lanes
// lane ^ 1, 2, 4 (wht_lanes): the lane with the bit clear holds a and keeps a + b, its partner holds b and keeps a - b.
// Every lane of a group must be here: H % 64 == 0 makes the col >= H early-out drop whole groups and a row's format
// is wave-uniform (what grp_pack8's max-abs shuffles rely on too).
template <class V>
__device__ __forceinline__ void wht8(V (&v)[8]) {
#pragma unroll
  for (int h = 1; h < 8; h <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (!(e & h)) {
        const V x = v[e], y = v[e + h];
        v[e] = x + y;
        v[e + h] = x - y;
      }
}
template <class V>
__device__ __forceinline__ void wht_lanes(V (&v)[8]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) {
    const bool up = lane & m;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const V o = __shfl_xor(v[e], m, 64);
      v[e] = up ? o - v[e] : v[e] + o;
    }
  }
}
// y = H64 v / 8 of a group (the encoder's rotation; the 1/8 is exact)
__device__ __forceinline__ void grp_rotate8(const float (&v)[8], float (&y)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = v[e];
  wht8(y);
  wht_lanes(y);
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] *= 0.125f;
}
__device__ __forceinline__ void grp_pack8_rot(uint8_t* __restrict__ row, const CodecArgs& a, int col,
                                              const float (&v)[8]) {
  float y[8];
  grp_rotate8(v, y);
  grp_pack8(row, a, col, y);
}
// As grp_unpack8 (NaN from the first bad group on), but a bad group - uniform over the group's 8 lanes - only zeroes
// the codes before the shuffles and is applied after them, so no lane of a group leaves early.
__device__ __forceinline__ void grp_unpack8_rot(const uint8_t* __restrict__ row, const CodecArgs& a, int col,
                                                float (&o)[8]) {
  const int lane = threadIdx.x & 63;
  const int g = col >> 6, sub = lane & 7;
  const GrpWalk k = grp_walk(a, g);
  const int bits = k.bits;
  int q[8];
  float s = 0.f;
  if (!k.bad) {
    const uint64_t w = grp_load(row + k.off + sub * bits, bits);
    s = *(const float*)(row + a.grp_code_bytes + 4 * g);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = grp_code(w, bits, e);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = 0;
  }
  wht8(q);
  wht_lanes(q);
  const float sc = s * 0.125f;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = k.bad ? __builtin_nanf("") : (float)q[e] * sc;
}

// FMT_F16 / FMT_F16S: 8 values <-> 4 words of two binary16 codes (even channel in the low half), each word its own
// 4-byte access (FMT_F16S rows are only 4-byte aligned); the conversions are the compiler's (round to nearest even,
// fp16 subnormals kept).
__device__ __forceinline__ void f16_store8(uint8_t* __restrict__ dst, const float (&v)[8], float inv) {
#pragma unroll
  for (int e = 0; e < 4; ++e) ((uint32_t*)dst)[e] = pack_h2(v[2 * e] * inv, v[2 * e + 1] * inv);
}
__device__ __forceinline__ void f16_load8(const uint8_t* __restrict__ src, float (&o)[8], float p) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f16x2_t h = __builtin_bit_cast(f16x2_t, ((const uint32_t*)src)[e]);
    o[2 * e] = (float)h[0] * p;
    o[2 * e + 1] = (float)h[1] * p;
  }
}
// The scale of an FMT_F16S row from the bits of its max|x| (see the header): p and inv = 1 / p.
struct F16Scale { float p, inv; };
__device__ __forceinline__ F16Scale f16s_scale(uint32_t amb) {
  const int E = (int)(amb >> 23);
  if (E == 255) return {__uint_as_float(amb), 1.f};   // NaN / Inf: p = a, every channel decodes non-finite
  if (amb == 0) return {1.f, 1.f};
  const int k = min(max(E - 141, -112), 113);
  return {__uint_as_float((uint32_t)(127 + k) << 23), __uint_as_float((uint32_t)(127 - k) << 23)};
}

// ---- MXFP6 rows: one lane per 32-channel block -----------------------------------------------------------------------
// A wave's LDS slice holds up to 4 chunks (512 channels each: the 8 channels of each of 64 lanes) of its row as fp32,
// MX6_PASS(NCH) chunks per pass (NCH 8: two passes).  Logical float index of channel ch of a pass: ch, in 16-byte
// slots s = ch / 4; block j = s / 8 owns slots 8 j .. 8 j + 7.  Two access patterns:
//   chunk layout: lane l, chunk c: slots 128 c + 2 l and + 1 (its 8 channels; two b128 accesses);
//   block layout: lane L = 16 c + j (chunk c's 16 blocks on lanes 16 c .. 16 c + 15): slots 8 L + i, i = 0 .. 7 (eight
//                 b128 accesses: the block's 32 consecutive floats).
// Bank model (64 banks of 4 bytes; a b128 access is served 16 lanes at a time, a lane covering the 4 banks of its slot,
// slot mod 16): plain, the block layout puts lane L's access i on slot 8 L + i - mod 16 only L's parity varies, a 8-way
// conflict within 16 lanes.  Swizzle: physical slot = s ^ ((j >> 1) & 7) with j = s >> 3 the slot's block - it permutes
// the 8 slots of a block among themselves, so a block stays in its 128 bytes.
//   block layout, access i: slot mod 16 = (i ^ ((L >> 1) & 7)) | (L & 1) << 3 - distinct for any 16 lanes with distinct
//     L mod 16 (contiguous lanes, or the non-contiguous b128 groups {0-3, 12-15, 20-27}, ...): conflict-free.
//   chunk layout, access e: j = 16 c + (l >> 2), so slot mod 16 = ((2 l + e) & 15) ^ ((l >> 3) & 7): lanes 8 m .. 8 m + 7
//     cover the 8 slots of one parity (e ^ m's low bit) and lanes 8 (m + 1) .. the other parity: conflict-free for 16
//     contiguous lanes and for the groups above.
// Only the wave touches its slice, so no workgroup barrier: a wave's LDS instructions execute in issue order, and the
// wavefront-scope fences (mx6_wave_sync) keep the compiler from moving one lane's reads above the stores of the others
// or the next pass's stores above this pass's reads.  A row's format is wave-uniform, so every lane is there.
constexpr int MX6_PASS(int nch) { return nch < 4 ? nch : 4; }
typedef __attribute__((ext_vector_type(16))) float f32v16_t;
typedef __attribute__((ext_vector_type(32))) float f32v32_t;
typedef __attribute__((ext_vector_type(6))) uint32_t u32x6_t;
__device__ __forceinline__ void mx6_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int mx6_chunk_slot(int c, int lane, int e) { return (128 * c + 2 * lane + e) ^ ((lane >> 3) & 7); }
__device__ __forceinline__ int mx6_block_slot(int L, int i) { return (8 * L + i) ^ ((L >> 1) & 7); }

// Rotated 6-bit rows: the lane owns the block, so the five stages of the unnormalised 32-point Walsh-Hadamard transform
// (strides 1, 2, 4, 8, 16, the lower index keeping the sum: 80 add / sub) run on its 32 values in place - X an array or
// a vector of 32 floats, in natural channel order.
template <class X>
__device__ __forceinline__ void wht32(X& x) {
#pragma unroll
  for (int h = 1; h < 32; h <<= 1)
#pragma unroll
    for (int e = 0; e < 32; ++e)
      if (!(e & h)) {
        const float a = x[e], b = x[e + h];
        x[e] = a + b;
        x[e + h] = a - b;
      }
}

// fmt: FMT_MXFP6 / FMT_MXBF6, the element type; R6: the row is the rotated twin's
template <int NCH, bool R6 = false>
__device__ __forceinline__ void mx6_pack_row(uint8_t* __restrict__ row, int H, int fmt, const float (&v)[NCH][8],
                                             float* __restrict__ slice) {
  constexpr int P = MX6_PASS(NCH);
  const int lane = threadIdx.x & 63, nblk = H / 32;
  const bool e2m3 = fmt == FMT_MXFP6;
#pragma unroll
  for (int p0 = 0; p0 < NCH; p0 += P) {
#pragma unroll
    for (int c = 0; c < P; ++c) {
      *(f32x4_t*)(slice + 4 * mx6_chunk_slot(c, lane, 0)) = f32x4_t{v[p0 + c][0], v[p0 + c][1], v[p0 + c][2], v[p0 + c][3]};
      *(f32x4_t*)(slice + 4 * mx6_chunk_slot(c, lane, 1)) = f32x4_t{v[p0 + c][4], v[p0 + c][5], v[p0 + c][6], v[p0 + c][7]};
    }
    mx6_wave_sync();
    const int blk = 16 * p0 + lane;          // the row's block on this lane
    if (lane < 16 * P && blk < nblk) {
      float x[32];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x4_t t = *(const f32x4_t*)(slice + 4 * mx6_block_slot(lane, i));
#pragma unroll
        for (int e = 0; e < 4; ++e) x[4 * i + e] = t[e];
      }
      if constexpr (R6) {   // y = H32 x / 4 of the natural-order block, before the even / odd split below
        wht32(x);
#pragma unroll
        for (int e = 0; e < 32; ++e) x[e] *= 0.25f;
      }
      uint32_t amb = 0;
#pragma unroll
      for (int e = 0; e < 32; ++e) amb = umax(amb, abs_bits(x[e]));
      const int sb = mx_scale_byte(__uint_as_float(amb), e2m3 ? 2 : 4);
      const float X = e8m0_value(sb == MX_NAN ? 127 : sb);   // the codes of a NaN block are never read
      const float lim = (e2m3 ? 7.5f : 28.f) * X;            // exact: a multiple of 2^-149 at X = 2^-127
      f32v16_t ev, od;                                       // operand 0: codes 0, 2, ...; operand 1: codes 1, 3, ...
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        ev[e] = __builtin_amdgcn_fmed3f(x[2 * e], -lim, lim);       // one v_med3_f32; a NaN is in a NaN block only
        od[e] = __builtin_amdgcn_fmed3f(x[2 * e + 1], -lim, lim);
      }
      const u32x6_t w = e2m3 ? __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(ev, od, X)
                             : __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(ev, od, X);
      u32_una_t* dst = (u32_una_t*)(row + 24 * blk);
#pragma unroll
      for (int i = 0; i < 6; ++i) dst[i] = w[i];
      row[24 * nblk + blk] = (uint8_t)sb;
    }
    if (p0 + P < NCH) mx6_wave_sync();
  }
}

// ---- Outlier rows: the 8 largest channels of a row, exactly ----------------------------------------------------------
// The wave-wide maximum of an unsigned value as a wave-uniform (scalar register) result, on the VALU's DPP operand
// path: an inclusive max-scan of each 16-lane row (row_shr 1, 2, 4, 8: a lane whose source lies outside its row keeps
// `old`, 0, the identity), the total of rows 0 / 2 into rows 1 / 3 (row_bcast15 under row mask 0xa), that of rows 0-1
// into rows 2-3 (row_bcast31 under row mask 0xc): lane 63 holds the maximum of all 64, read with v_readlane_b32.  Six
// v_max_u32 with a DPP operand against wave_umax's six ds_bpermute_b32 round trips through the LDS crossbar, and the
// result is scalar: compares take it as a scalar operand and what is derived from it (the winner's chunk, element and
// lane) is wave-uniform, so the branches on it are scalar branches.  Every lane of the wave must be active.
enum { DPP_ROW_SHR = 0x110, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143 };
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dpp_umax(uint32_t x) {
  return umax(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ uint32_t wave_umax_s(uint32_t x) {
  x = dpp_umax<DPP_ROW_SHR + 1>(x);
  x = dpp_umax<DPP_ROW_SHR + 2>(x);
  x = dpp_umax<DPP_ROW_SHR + 4>(x);
  x = dpp_umax<DPP_ROW_SHR + 8>(x);
  x = dpp_umax<DPP_ROW_BCAST15, 0xa>(x);
  x = dpp_umax<DPP_ROW_BCAST31, 0xc>(x);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint32_t lane_bits(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); }

// A lane's best live element of one chunk.  key: bits | 2^31 of a live element (above every taken one, ordered by
// abs_bits), 0 of a taken one - bit e of `taken` set: element e has left the row, or lies past H.  The first of equal
// keys wins (ascending e: the lower channel).  kr = 512 c + e, the element's channel less 8 lane.
__device__ __forceinline__ void out_scan8(const float (&v)[8], uint32_t taken, int c, uint32_t& ka, uint32_t& kr) {
  ka = 0;
  kr = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t key = (taken >> e) & 1u ? 0u : (__float_as_uint(v[e]) | 0x80000000u);
    if (key > ka) { ka = key; kr = (uint32_t)(c * 512 + e); }
  }
}
// pack_kernel's selection for an outlier row, held as everywhere 8 consecutive channels per lane and chunk in
// v[NCH][8]: writes the row's tail ([8 fp32 values][8 uint16 channels] at `tail`, lanes 0 .. 7, pair r on lane r),
// replaces the 8 channels by +0 in v and returns the bits of the max|x| of the rest.  No LDS, no scratch, no register
// indexed by data.  The split that was built: every lane caches, per chunk, its best live (key, place) pair, so a round
// is (1) the lane's best over its NCH cached pairs, (2) two wave_umax_s - the key, then ~channel among the lanes
// holding it: the lowest such channel - which give the winner wave-uniformly, (3) under scalar branches on the winner's
// chunk: its exact bits (a select over the chunk's 8 registers by the uniform element index, read from the owning lane
// with v_readlane_b32), its bit in the owner's `taken` mask, and a rescan of THAT chunk's 8 registers only.  The
// registers themselves stay as loaded until the 8 rounds are over - a taken element is masked, not zeroed, so a zero
// that was taken cannot win again against the live zeros of an all-zero rest - and the rescan runs on all lanes
// unpredicated: only the owner's mask changed, every other lane recomputes what it had, at the same issue cost as a
// predicated one.  A round so rescans 8 registers, not the lane's 8 NCH.  A lane-local pre-selection of 8 candidates
// (fewer wave-wide rounds) was not built: it needs a sorted insert per element, 8 compares each.
// After round 8 the cached keys are those of the rest: one more wave_umax_s is its max-abs, with no second pass.
// Channels past H (a partial last chunk: zeros in v) start as taken; H >= 32 leaves at least 24 live channels.
template <int NCH>
__device__ __forceinline__ uint32_t out_extract(float (&v)[NCH][8], int H, uint8_t* __restrict__ tail) {
  const int lane = threadIdx.x & 63;
  uint32_t taken[(NCH + 3) / 4], ca[NCH], cr[NCH];   // taken: 8 bits a chunk, 4 chunks a word
#pragma unroll
  for (int w = 0; w < (NCH + 3) / 4; ++w) taken[w] = 0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if ((c * 64 + lane) * 8 >= H) taken[c >> 2] |= 0xffu << (8 * (c & 3));
    out_scan8(v[c], taken[c >> 2] >> (8 * (c & 3)), c, ca[c], cr[c]);
  }
  uint32_t myval = 0, myidx = 0;
#pragma unroll
  for (int r = 0; r < OUT_K; ++r) {
    uint32_t ka = ca[0], kr = cr[0];
#pragma unroll
    for (int c = 1; c < NCH; ++c)
      if (ca[c] > ka) { ka = ca[c]; kr = cr[c]; }
    const uint32_t m = wave_umax_s(ka);
    const uint32_t win = ~wave_umax_s(ka == m ? ~((uint32_t)lane * 8 + kr) : 0u);   // the winner's channel
    const int wc = (int)(win >> 9), we = (int)(win & 7), wl = (int)(win >> 3) & 63;
    uint32_t val = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (wc != c) continue;
      float x = v[c][0];
#pragma unroll
      for (int e = 1; e < 8; ++e) x = we == e ? v[c][e] : x;
      val = lane_bits(__float_as_uint(x), wl);
      if (lane == wl) taken[c >> 2] |= 1u << (8 * (c & 3) + we);
      out_scan8(v[c], taken[c >> 2] >> (8 * (c & 3)), c, ca[c], cr[c]);
    }
    if (lane == r) { myval = val; myidx = win; }
  }
  uint32_t ka = ca[0];
#pragma unroll
  for (int c = 1; c < NCH; ++c) ka = umax(ka, ca[c]);
  const uint32_t amb = wave_umax_s(ka) & 0x7fffffffu;   // no live element on any lane: 0
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if ((taken[c >> 2] >> (8 * (c & 3) + e)) & 1u) v[c][e] = 0.f;
  if (lane < OUT_K) {
    *(uint32_t*)(tail + 4 * lane) = myval;
    *(uint16_t*)(tail + 4 * OUT_K + 2 * lane) = (uint16_t)myidx;
  }
  return amb;
}

// unpack_kernel's side: the 8 (channel, value) pairs of a row's tail, read once by lanes 0 .. 7 and held wave-uniformly
// (v_readlane_b32 with constant lanes: 16 scalar registers), and `bad`: a channel >= H among them - the row decodes to
// NaN.  out_patch overwrites, in the 8 decoded values of chunk c on this lane, the channels of the pairs that lie in
// that chunk - a scalar branch per pair, then 8 compares of the pair's place on the lane against constants - in pair
// order, so the last of two pairs naming one channel holds, as on the CPU.  It runs before the chunk's store8: no
// address is formed from a message's channel, and nothing is stored twice.
struct OutPairs { uint32_t idx[OUT_K], val[OUT_K]; bool bad; };
__device__ __forceinline__ OutPairs out_load(const uint8_t* __restrict__ tail, int H) {
  const int lane = threadIdx.x & 63;
  uint32_t val = 0, idx = 0;
  if (lane < OUT_K) {
    val = *(const uint32_t*)(tail + 4 * lane);
    idx = *(const uint16_t*)(tail + 4 * OUT_K + 2 * lane);
  }
  OutPairs p;
  p.bad = false;
#pragma unroll
  for (int r = 0; r < OUT_K; ++r) {
    p.idx[r] = lane_bits(idx, r);
    p.val[r] = lane_bits(val, r);
    p.bad |= p.idx[r] >= (uint32_t)H;
  }
  return p;
}
__device__ __forceinline__ void out_patch(float (&o)[8], const OutPairs& p, int c) {
  const uint32_t base = (uint32_t)(c * 64 + (threadIdx.x & 63)) * 8;
#pragma unroll
  for (int r = 0; r < OUT_K; ++r) {
    if ((int)(p.idx[r] >> 9) != c) continue;
    const uint32_t at = p.idx[r] - base;   // 0 .. 7 on the lane holding the channel
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = at == (uint32_t)e ? __uint_as_float(p.val[r]) : o[e];
  }
  if (p.bad) fill8(o, __builtin_nanf(""));
}

// ---- Row-rotated per-token int rows: one Hadamard transform of the whole row ------------------------------------------
// The wave holds the row as everywhere else: v[NCH][8], channel = (64 c + lane) 8 + e.
// H = 2^n, registers and cross-lane moves only: strides 1 .. 64 are wht_row16 per chunk; stride 128 pairs lane ^ 16 and
// stride 256 lane ^ 32 (wht_xrow: v_permlane16_swap / v_permlane32_swap of a value with itself hand every lane the pair
// (even side, odd side) - the lane with the stride bit set holds the odd side, negates it, and both add); strides 512,
// 1024, 2048 are butterflies between the chunk registers v[c] and v[c ^ 1], v[c ^ 2], v[c ^ 4].  A stage whose stride
// is not below H is skipped on a wave-uniform condition.  Every lane is at the moves: chunks and lanes past H hold
// zeros and rotate zeros among themselves (a pair of lanes or chunks is past H together or not at all).
template <bool X32>
__device__ __forceinline__ void wht_xrow(float (&v)[8]) {   // the butterfly between lanes l and l ^ 16 (X32: l ^ 32)
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t sg = X32 ? (lane & 32u) << 26 : (lane & 16u) << 27;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t u = __float_as_uint(v[e]);
    const auto r = X32 ? __builtin_amdgcn_permlane32_swap(u, u, false, false)
                       : __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v[e] = __uint_as_float(r[0]) + __uint_as_float(r[1] ^ sg);   // r[0]: the side with the bit clear, r[1]: with it set
  }
}
__device__ __forceinline__ void wht_lane4(float (&v)[8]) {   // the butterfly between lanes l and l ^ 4 (wht_row16's)
  const uint32_t s4 = (threadIdx.x & 4u) << 29;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t u = __float_as_uint(v[e]);
    v[e] = __uint_as_float(quad_mov<DPP_QUAD_REV>(quad_mov<DPP_ROW_HALF_MIRROR>(u))) + __uint_as_float(u ^ s4);
  }
}
template <int NCH>
__device__ __forceinline__ void wht_pow2_row(float (&v)[NCH][8], int H) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) wht_row16(v[c]);
  if (H > 128) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) wht_xrow<false>(v[c]);
  }
  if (H > 256) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) wht_xrow<true>(v[c]);
  }
#pragma unroll
  for (int h = 1; h < NCH; h <<= 1) {
    if (H <= 512 * h) continue;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c & h) continue;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = v[c][e], y = v[c + h][e];
        v[c][e] = x + y;
        v[c + h][e] = x - y;
      }
    }
  }
}

// H = 28 2^m.  The signs of H28, at compile time from the Paley construction for q = 13: chi the quadratic character mod
// 13, Q[i][j] = chi(i - j), C = [[0, 1'], [1, Q]] (14 x 14, symmetric as 13 = 1 mod 4, zero diagonal),
// H28 = C (x) [[1, 1], [1, -1]] + I14 (x) [[1, -1], [-1, -1]]: entries +-1, symmetric, H28 H28 = 28 I.
struct H28Signs { signed char s[28][28]; };
constexpr int chi13(int x) {
  x = (x % 13 + 13) % 13;
  if (x == 0) return 0;
  for (int k = 1; k < 13; ++k)
    if (k * k % 13 == x) return 1;
  return -1;
}
constexpr H28Signs make_h28() {
  H28Signs t{};
  for (int i = 0; i < 14; ++i)
    for (int j = 0; j < 14; ++j) {
      const int c = i == 0 && j == 0 ? 0 : i == 0 || j == 0 ? 1 : chi13(i - j);
      for (int r = 0; r < 2; ++r)
        for (int q = 0; q < 2; ++q)
          t.s[2 * i + r][2 * j + q] = (signed char)(c * (r && q ? -1 : 1) + (i == j ? (r || q ? -1 : 1) : 0));
    }
  return t;
}
// out = sum_a H28[I][a] t[a], in ascending a from +-t[0].  I and the a's are template constants, so every sign is a
// constant expression and the stage is 27 plain adds / subtracts per output: no table in memory, no register indexed
// by data.
template <int I, int... A>
__device__ __forceinline__ float h28_dot(const float (&t)[28], std::integer_sequence<int, A...>) {
  constexpr H28Signs S = make_h28();
  float acc = S.s[I][0] > 0 ? t[0] : -t[0];
  ((acc = S.s[I][A + 1] > 0 ? acc + t[A + 1] : acc - t[A + 1]), ...);
  return acc;
}
// o[i] = row BASE + (i ^ XR) of H28 t, i = 0 .. N - 1
template <int BASE, int XR, int... I>
__device__ __forceinline__ void h28_rows(const float (&t)[28], float (&o)[sizeof...(I)], std::integer_sequence<int, I...>) {
  ((o[I] = h28_dot<BASE + (I ^ XR)>(t, std::make_integer_sequence<int, 27>{})), ...);
}

// The 28-point stage runs along a, at stride 2^m channels, so the row goes through a per-wave LDS slice of H floats in
// natural channel order (float index = channel): written as the lanes hold it (two b128 per chunk), read back by
// column - b32 reads of t[a] = slice[a 2^m + b] for a = 0 .. 27 -, the outputs written back the same way and the
// lane-linear image read again (two b128 per chunk).  The 2^m columns over the 64 lanes:
//   m = 5 (NCH 2): two lanes per column, b = lane & 31; both read all 28 inputs, lane half h = lane >> 5 computes the 14
//          outputs a' = 14 h .. 14 h + 13 (the two halves run different signs, so they take the two sides of one branch);
//   m = 6 (NCH 4): one lane per column, b = lane;
//   m = 7 (NCH 8): two columns per lane, b = lane and lane + 64, one after the other.
// Bank model (64 banks of 4 bytes; a b32 access is conflict-free when its 64 lanes hit 64 banks or share an address, a
// b128 access is served 16 lanes at a time, a lane covering the 4 banks of its 16-byte slot, slot mod 16):
//   column reads: bank = (a 2^m + b) mod 64.  m = 6, 7: b mod 64 = lane - 64 banks.  m = 5: lanes l and l + 32 read one
//     address (a broadcast), the 32 columns hit banks 32 (a & 1) + b - conflict-free.
//   column writes: m = 6, 7 as the reads.  m = 5: with o[i] = output 14 h + i the halves would write addresses 448
//     floats = 14 * 128 B = 0 mod 256 B apart - the same bank, 2-way.  So half 1 holds its outputs pairwise swapped,
//     o[i] = output 14 + (i ^ 1): write i goes to banks 32 (i & 1) + b for half 0 and 32 (~i & 1) + b for half 1 -
//     conflict-free.
//   chunk accesses: lane l's slots are 2 (64 c + l) and + 1; taken in that order, lanes l and l + 8 of a 16-lane group
//     collide (slot mod 16 = 2 l mod 16), 2-way.  So lanes with bit 3 set take their two slots in the other order: access
//     k touches slot 2 l + (k ^ ((l >> 3) & 1)), lanes 0 - 7 of a group cover the 8 slots of one parity and lanes 8 - 15
//     those of the other - conflict-free.
// Only the wave touches its slice: no workgroup barrier; the wavefront-scope fences of mx6_wave_sync order one lane's
// accesses against the others'.  A lane's own column (m = 6, 7) is read and written by that lane alone, in program
// order.  Lanes whose channels lie past H take no part in the chunk accesses and keep their zeros.
constexpr int RF_M(int nch) { return nch == 2 ? 5 : nch == 4 ? 6 : 7; }
template <int NCH>
__device__ __forceinline__ void h28_stage_lds(float (&v)[NCH][8], int H, float* __restrict__ slice) {
  constexpr int M = RF_M(NCH), W = 1 << M;
  const int lane = threadIdx.x & 63;
  const bool flip = (lane >> 3) & 1;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col >= H) continue;
    const f32x4_t lo = {v[c][0], v[c][1], v[c][2], v[c][3]}, hi = {v[c][4], v[c][5], v[c][6], v[c][7]};
    *(f32x4_t*)(slice + col + (flip ? 4 : 0)) = flip ? hi : lo;
    *(f32x4_t*)(slice + col + (flip ? 0 : 4)) = flip ? lo : hi;
  }
  mx6_wave_sync();
  if constexpr (M == 5) {
    const int b = lane & 31, half = lane >> 5;
    float t[28], o[14];
#pragma unroll
    for (int a = 0; a < 28; ++a) t[a] = slice[a * W + b];
    if (half) h28_rows<14, 1>(t, o, std::make_integer_sequence<int, 14>{});
    else h28_rows<0, 0>(t, o, std::make_integer_sequence<int, 14>{});
    mx6_wave_sync();   // the column's other lane has read it
    // o[i] is output 14 half + (i ^ half): even i at row 14 half + i + half, odd i at 14 half + i - half
    float* pe = slice + (14 * half + half) * W + b;
    float* po = slice + (14 * half - half) * W + b;
#pragma unroll
    for (int i = 0; i < 14; ++i) (i & 1 ? po : pe)[i * W] = o[i];
  } else {
#pragma unroll
    for (int j = 0; j < W / 64; ++j) {
      float* p = slice + 64 * j + lane;
      float t[28], o[28];
#pragma unroll
      for (int a = 0; a < 28; ++a) t[a] = p[a * W];
      h28_rows<0, 0>(t, o, std::make_integer_sequence<int, 28>{});
#pragma unroll
      for (int a = 0; a < 28; ++a) p[a * W] = o[a];
    }
  }
  mx6_wave_sync();
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col >= H) continue;
    const f32x4_t x0 = *(const f32x4_t*)(slice + col + (flip ? 4 : 0));
    const f32x4_t x1 = *(const f32x4_t*)(slice + col + (flip ? 0 : 4));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[c][e] = flip ? x1[e] : x0[e];
      v[c][4 + e] = flip ? x0[e] : x1[e];
    }
  }
}
// The 2^m-point part along b, in the lanes that hold a block: 32 channels = a quad, 64 = 8 lanes, 128 = a DPP row.
template <int M>
__device__ __forceinline__ void wht_2m(float (&v)[8]) {
  if constexpr (M == 7) {
    wht_row16(v);
  } else {
    wht8(v);
    wht_quad(v);
    if constexpr (M == 6) wht_lane4(v);
  }
}
// floats of a wave's slice: a 28 2^m row exists at NCH 2, 4, 8 only (H = 896, 1792, 3584)
constexpr int RF_SLICE(int nch) { return nch > 1 ? 28 << RF_M(nch) : 4; }
// v <- H v, unnormalised.  DEC: the decoder's order (the 28-point stage first; on integer codes every order is exact).
template <int NCH, bool DEC>
__device__ __forceinline__ void rot_full_row(float (&v)[NCH][8], int H, float* __restrict__ slice) {
  if constexpr (NCH > 1) {
    if (H & (H - 1)) {   // wave-uniform: 28 2^m
      if constexpr (!DEC) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) wht_2m<RF_M(NCH)>(v[c]);
      }
      h28_stage_lds<NCH>(v, H, slice);
      if constexpr (DEC) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) wht_2m<RF_M(NCH)>(v[c]);
      }
      return;
    }
  }
  wht_pow2_row<NCH>(v, H);
}
// e and d of the comment at is_rf_fmt: ctz(H) = n, or m + 2
__device__ __forceinline__ float pow2f(int k) { return __uint_as_float((uint32_t)(127 + k) << 23); }
__device__ __forceinline__ float rf_enc_scale(int H) {
  const int n = __builtin_ctz(H);
  return H & (H - 1) ? pow2f(-(2 + (n - 2) / 2)) : pow2f(-(n / 2));
}
__device__ __forceinline__ float rf_dec_scale(int H) {
  const int n = __builtin_ctz(H);
  return H & (H - 1) ? (1.0f / 28.0f) * pow2f(2 - (n - 1) / 2) : pow2f(-((n + 1) / 2));
}

template <int NCH, class T, bool ROT = false, bool W16 = false, bool MX6 = false, bool MXR = false, bool OUT = false,
          bool RR = false, bool RF = false, bool NV4 = false>
__global__ __launch_bounds__(256) void pack_kernel(CodecArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.S) return;
  const int lane = threadIdx.x & 63;
  const RowSlot rs = row_slot<ROT, W16, MX6, MXR, OUT, RR, RF, NV4>(a, row);
  uint8_t* dst = rs.p;
  const bool orow = OUT && is_out_fmt(rs.fmt);   // an outlier row: fmt is its plain twin's
  const bool rrow = RR && is_rr_fmt(rs.fmt);     // a rotated int row: fmt is its plain twin's
  const bool frow = RF && is_rf_fmt(rs.fmt);     // a row-rotated int row: the same
  const int fmt = rf_twin<RF>(rr_twin<RR>(out_twin<OUT>(rs.fmt))), qmax = rs.qmax, b = rs.b;
  float v[NCH][8];
  load_row8<NCH>((const T*)a.x + (size_t)row * a.H, a.H, v);
  float* scales = (float*)(a.msg + a.off_scale);
  if constexpr (RR) {   // a rotated int row: v becomes y = H128 x / 8, all 64 lanes and all chunks at the moves (chunks
    if (rrow) {         // past H rotate zeros to zeros); from here on the row is its plain twin's
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        wht_row16(v[c]);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[c][e] *= 0.125f;
      }
    }
  }
  if constexpr (RF) {   // a row-rotated int row: v becomes y = e H x of the whole row; from here on it is its plain twin's
    __shared__ __attribute__((aligned(16))) float rf_lds[4][RF_SLICE(NCH)];
    if (frow) {         // wave-uniform: the row's format
      rot_full_row<NCH, false>(v, a.H, rf_lds[threadIdx.x >> 6]);
      const float es = rf_enc_scale(a.H);
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[c][e] *= es;
    }
  }

  // scale / quantiser for this row
  float inv = 0.f, mul = 0.f;  // code = round(x * inv) for token & channel; window mode uses ref formula
  const bool raw = SELF_SCALED(ROT, W16, MX6, MXR, NV4, fmt);
  if (raw && a.scale_mode == SC_TOKEN && lane == 0) scales[row] = 0.f;
  if (!raw) {
    if (a.scale_mode == SC_TOKEN) {
      uint32_t amb = 0;
      if constexpr (OUT) {   // an outlier row: its 8 outliers leave v for the row's tail, the max-abs is the rest's
        if (orow) {
          amb = out_extract<NCH>(v, a.H, dst + fmt_row_bytes<false, false>(fmt, a.H));
        } else {
#pragma unroll
          for (int c = 0; c < NCH; ++c) amb = umax(amb, umax8(v[c]));
          amb = wave_umax(amb);
        }
      } else {
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) amb = umax(amb, abs_bits(v[c][e]));
        amb = wave_umax(amb);
      }
      const float am = __uint_as_float(amb);   // NaN / Inf if the row (an outlier row: its rest) holds one: s non-finite
      const float s = tok_scale(am, qmax);
      if (lane == 0) scales[row] = s;
      inv = tok_inv(am, s);
    } else if (a.scale_mode == SC_WINDOW) {
      mul = scales[b];  // max|x| over the window's lo rows
    }
  }
  if constexpr (MX6) {
    __shared__ __attribute__((aligned(16))) float mx6_lds[4][MX6_PASS(NCH) * 512];
    if (fmt == FMT_MXFP6 || fmt == FMT_MXBF6) {   // wave-uniform: the row's format
      mx6_pack_row<NCH>(dst, a.H, fmt, v, mx6_lds[threadIdx.x >> 6]);
      return;
    }
    if constexpr (MXR) {
      if (fmt == FMT_MXFP6R || fmt == FMT_MXBF6R) {
        mx6_pack_row<NCH, true>(dst, a.H, fmt == FMT_MXFP6R ? FMT_MXFP6 : FMT_MXBF6, v, mx6_lds[threadIdx.x >> 6]);
        return;
      }
    }
  }
  const float qmaxf = (float)qmax;
  const float qminf = qmin_of(a.scale_mode, qmax);
  float inv16 = 1.f;   // FMT_F16S: 1 / p of the row (FMT_F16: 1, an exact multiply)
  if constexpr (W16) {
    if (fmt == FMT_F16S) {
      uint32_t amb = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) amb = umax(amb, umax8(v[c]));
      const F16Scale k = f16s_scale(wave_umax(amb));
      inv16 = k.inv;
      if (lane == 0) *(float*)(dst + 2 * a.H) = k.p;
    }
  }
  float nvg = 0.f;     // FMT_NVFP4: the row's second-level scale g
  if constexpr (NV4) {
    if (fmt == FMT_NVFP4) {
      uint32_t amb = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) amb = umax(amb, umax8(v[c]));
      nvg = nv_row_scale(wave_umax(amb));
      if (lane == 0) *(f32_una_t*)(dst + 9 * (a.H / 16)) = nvg;
    }
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col >= a.H) continue;
    int q[8];
    if (fmt == FMT_F32) {
      *(f32x4_t*)(dst + col * 4) = f32x4_t{v[c][0], v[c][1], v[c][2], v[c][3]};
      *(f32x4_t*)(dst + col * 4 + 16) = f32x4_t{v[c][4], v[c][5], v[c][6], v[c][7]};
      continue;
    }
    if (fmt == FMT_MXFP4 || fmt == FMT_MXFP8) {
      mx_pack8(dst, a.H, col, fmt, v[c]);
      continue;
    }
    if constexpr (MXR) {   // all 4 lanes of the block's quad are here (wht_quad)
      if (fmt == FMT_MXFP4R || fmt == FMT_MXFP8R) {
        mx_pack8_rot(dst, a.H, col, fmt == FMT_MXFP4R ? FMT_MXFP4 : FMT_MXFP8, v[c]);
        continue;
      }
    }
    if constexpr (NV4) {   // both lanes of the block's pair are here (nv_pack8)
      if (fmt == FMT_NVFP4) {
        nv_pack8(dst, a.H, col, v[c], nvg);
        continue;
      }
    }
    if (fmt == FMT_GRP) {
      grp_pack8(dst, a, col, v[c]);
      continue;
    }
    if constexpr (ROT) {
      if (fmt == FMT_GRPR) {
        grp_pack8_rot(dst, a, col, v[c]);
        continue;
      }
    }
    if (fmt == FMT_BF16) {
      u32x4_t w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = pack_bf2(v[c][2 * e], v[c][2 * e + 1]);
      *(u32x4_t*)(dst + col * 2) = w;
      continue;
    }
    if constexpr (W16) {
      if (fmt == FMT_F16 || fmt == FMT_F16S) {
        f16_store8(dst + col * 2, v[c], inv16);
        continue;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xv = v[c][e];
      float t;
      if (a.scale_mode == SC_TOKEN) {
        t = tok_code(xv, inv, qmaxf, qminf);
      } else if (a.scale_mode == SC_WINDOW) {
        t = win_code(xv, mul, qmaxf, qminf);
      } else {
        const float sc = scales[(size_t)b * a.H + col + e];
        if (a.ch_kind == CH_MEAN || qmax == 1) {
          t = sc != 0.f ? fminf(fmaxf(rintf(xv / sc), -1.f), 1.f) : 0.f;       // ternary (reference clamps)
        } else {
          t = sc > 0.f ? rintf(xv / sc * qmaxf) : 0.f;                         // reference: no clamp
        }
      }
      q[e] = (int)t;
    }
    if (fmt == FMT_INT8) {
      u32x2_t w;
      w[0] = (q[0] & 255) | ((q[1] & 255) << 8) | ((q[2] & 255) << 16) | ((uint32_t)(q[3] & 255) << 24);
      w[1] = (q[4] & 255) | ((q[5] & 255) << 8) | ((q[6] & 255) << 16) | ((uint32_t)(q[7] & 255) << 24);
      *(u32x2_t*)(dst + col) = w;
    } else if (fmt == FMT_INT4) {
      uint32_t w = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) w |= (uint32_t)(q[e] & 15) << (4 * e);
      *(uint32_t*)(dst + col / 2) = w;
    } else {
      uint32_t w = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) w |= (uint32_t)(q[e] & 3) << (2 * e);
      *(uint16_t*)(dst + col / 4) = (uint16_t)w;
    }
  }
}

__device__ __forceinline__ void store8(bf16_t* dst, const float (&o)[8]) {
  u32x4_t w;
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = pack_bf2(o[2 * e], o[2 * e + 1]);
  *(u32x4_t*)dst = w;
}
__device__ __forceinline__ void store8(float* dst, const float (&o)[8]) {
  *(f32x4_t*)dst = f32x4_t{o[0], o[1], o[2], o[3]};
  *(f32x4_t*)(dst + 4) = f32x4_t{o[4], o[5], o[6], o[7]};
}

// The 8 integer codes at channels col .. col + 7 of an FMT_INT8 / FMT_INT4 / FMT_INT2 row, as unpack_kernel's own loop
// reads them (which keeps its inline copy: through this function its instantiations compile to other code)
__device__ __forceinline__ void int_codes8(const uint8_t* __restrict__ src, int col, int fmt, int (&q)[8]) {
  if (fmt == FMT_INT8) {
    const u32x2_t w = *(const u32x2_t*)(src + col);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      q[e] = (int)(int8_t)((w[0] >> (8 * e)) & 255);
      q[4 + e] = (int)(int8_t)((w[1] >> (8 * e)) & 255);
    }
  } else if (fmt == FMT_INT4) {
    const uint32_t w = *(const uint32_t*)(src + col / 2);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = ((int)(w << (28 - 4 * e))) >> 28;
  } else {
    const uint32_t w = *(const uint16_t*)(src + col / 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = ((int)(w << (30 - 2 * e))) >> 30;
  }
}

// A row-rotated int row: x' = (s d) H q.  The whole row - the codes of all its chunks as floats, zeros past H - is in
// registers before the stages run, so there is no store per chunk as for the other formats; the data flow mirrors
// pack's (rot_full_row, the decoder's order), one multiply, then the row's store8s.  fmt: the plain twin's.
template <int NCH, class T>
__device__ __forceinline__ void rf_unpack_row(const uint8_t* __restrict__ src, int H, int fmt, float s,
                                              T* __restrict__ out, float* __restrict__ slice) {
  const int lane = threadIdx.x & 63;
  float o[NCH][8];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    int q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < H) int_codes8(src, col, fmt, q);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[c][e] = (float)q[e];
  }
  rot_full_row<NCH, true>(o, H, slice);
  const float sc = s * rf_dec_scale(H);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col >= H) continue;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[c][e] *= sc;
    store8(out + col, o[c]);
  }
}

template <int NCH, class T, bool R6 = false>
__device__ __forceinline__ void mx6_unpack_row(const uint8_t* __restrict__ row, int H, int fmt, T* __restrict__ out,
                                               float* __restrict__ slice) {
  constexpr int P = MX6_PASS(NCH);
  const int lane = threadIdx.x & 63, nblk = H / 32;
#pragma unroll
  for (int p0 = 0; p0 < NCH; p0 += P) {
    const int blk = 16 * p0 + lane;
    if (lane < 16 * P && blk < nblk) {
      const u32_una_t* src = (const u32_una_t*)(row + 24 * blk);
      u32x6_t w;
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i] = src[i];
      const int sb = row[24 * nblk + blk];
      const float X = e8m0_value(sb == MX_NAN ? 127 : sb);
      f32v32_t x = fmt == FMT_MXFP6 ? __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(w, X)
                                    : __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(w, X);
      if constexpr (R6) {   // x' = H32 y' / 8 (a NaN block's values are replaced below all the same)
        wht32(x);
#pragma unroll
        for (int e = 0; e < 32; ++e) x[e] *= 0.125f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        f32x4_t t;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = sb == MX_NAN ? __builtin_nanf("") : x[4 * i + e];
        *(f32x4_t*)(slice + 4 * mx6_block_slot(lane, i)) = t;
      }
    }
    mx6_wave_sync();
#pragma unroll
    for (int c = 0; c < P; ++c) {
      const int col = ((p0 + c) * 64 + lane) * 8;
      if (col >= H) continue;
      const f32x4_t t0 = *(const f32x4_t*)(slice + 4 * mx6_chunk_slot(c, lane, 0));
      const f32x4_t t1 = *(const f32x4_t*)(slice + 4 * mx6_chunk_slot(c, lane, 1));
      const float o[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
      store8(out + col, o);
    }
    if (p0 + P < NCH) mx6_wave_sync();
  }
}

template <int NCH, class T, bool ROT = false, bool W16 = false, bool MX6 = false, bool MXR = false, bool OUT = false,
          bool RR = false, bool RF = false, bool NV4 = false>
__global__ __launch_bounds__(256) void unpack_kernel(CodecArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.S) return;
  const int lane = threadIdx.x & 63;
  const RowSlot rs = row_slot<ROT, W16, MX6, MXR, OUT, RR, RF, NV4>(a, row);
  const uint8_t* src = rs.p;
  const bool orow = OUT && is_out_fmt(rs.fmt);   // an outlier row: fmt is its plain twin's
  const bool rrow = RR && is_rr_fmt(rs.fmt);     // a rotated int row: fmt is its plain twin's
  const bool frow = RF && is_rf_fmt(rs.fmt);     // a row-rotated int row: the same
  const int fmt = rf_twin<RF>(rr_twin<RR>(out_twin<OUT>(rs.fmt))), qmax = rs.qmax, b = rs.b;
  const float* scales = (const float*)(a.msg + a.off_scale);
  float s = 0.f;
  if (!SELF_SCALED(ROT, W16, MX6, MXR, NV4, fmt)) {
    if (a.scale_mode == SC_TOKEN) s = scales[row];
    else if (a.scale_mode == SC_WINDOW) s = scales[b];
  }
  T* out = (T*)a.x + (size_t)row * a.H;
  if constexpr (MX6 || MXR || OUT || RR || RF || NV4) {
    // header word 7 of a message with 6-bit, rotated, outlier or NVFP4 rows names both classes' formats; one that disagrees with the
    // formats this launch was given (encoded with another element type, or without the modifier) decodes to NaN - loud
    if (((const int*)a.msg)[7] != (a.hi_fmt | a.lo_fmt << 8)) {
      float o[8];
      fill8(o, __builtin_nanf(""));
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = (c * 64 + lane) * 8;
        if (col < a.H) store8(out + col, o);
      }
      return;
    }
  }
  if constexpr (MX6) {
    __shared__ __attribute__((aligned(16))) float mx6_lds[4][MX6_PASS(NCH) * 512];
    if (fmt == FMT_MXFP6 || fmt == FMT_MXBF6) {   // wave-uniform: the row's format
      mx6_unpack_row<NCH>(src, a.H, fmt, out, mx6_lds[threadIdx.x >> 6]);
      return;
    }
    if constexpr (MXR) {
      if (fmt == FMT_MXFP6R || fmt == FMT_MXBF6R) {
        mx6_unpack_row<NCH, T, true>(src, a.H, fmt == FMT_MXFP6R ? FMT_MXFP6 : FMT_MXBF6, out,
                                     mx6_lds[threadIdx.x >> 6]);
        return;
      }
    }
  }
  if constexpr (RF) {
    __shared__ __attribute__((aligned(16))) float rf_lds[4][RF_SLICE(NCH)];
    if (frow) {   // wave-uniform: the row's format
      rf_unpack_row<NCH>(src, a.H, fmt, s, out, rf_lds[threadIdx.x >> 6]);
      return;
    }
  }
  float p16 = 1.f;   // FMT_F16S: the row's p (FMT_F16: 1, an exact multiply)
  if constexpr (W16) {
    if (fmt == FMT_F16S) p16 = *(const float*)(src + 2 * a.H);
  }
  OutPairs op;
  if constexpr (OUT) {
    if (orow) op = out_load(src + fmt_row_bytes<false, false>(fmt, a.H), a.H);   // wave-uniform: the row's format
  }
  float nvg = 0.f;     // FMT_NVFP4: the row's second-level scale g
  if constexpr (NV4) {
    if (fmt == FMT_NVFP4) nvg = nv_load_scale(src, a.H);
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col >= a.H) continue;
    if constexpr (W16) {
      if (fmt == FMT_F16 || fmt == FMT_F16S) {
        float o[8];
        f16_load8(src + col * 2, o, p16);
        store8(out + col, o);
        continue;
      }
    }
    if (fmt == FMT_BF16 || fmt == FMT_F32) {
      float o[8];
      if (fmt == FMT_F32) {
        const f32x4_t x0 = *(const f32x4_t*)(src + col * 4), x1 = *(const f32x4_t*)(src + col * 4 + 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = x0[e]; o[4 + e] = x1[e]; }
      } else {
        const u32x4_t w = *(const u32x4_t*)(src + col * 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[2 * e] = bf_lo(w[e]); o[2 * e + 1] = bf_hi(w[e]); }
      }
      store8(out + col, o);
      continue;
    }
    if (fmt == FMT_MXFP4 || fmt == FMT_MXFP8) {
      float o[8];
      mx_unpack8(src, a.H, col, fmt, o);
      store8(out + col, o);
      continue;
    }
    if constexpr (MXR) {   // all 4 lanes of the block's quad are here (wht_quad)
      if (fmt == FMT_MXFP4R || fmt == FMT_MXFP8R) {
        float o[8];
        mx_unpack8_rot(src, a.H, col, fmt == FMT_MXFP4R ? FMT_MXFP4 : FMT_MXFP8, o);
        store8(out + col, o);
        continue;
      }
    }
    if constexpr (NV4) {
      if (fmt == FMT_NVFP4) {
        float o[8];
        nv_unpack8(src, a.H, col, nvg, o);
        store8(out + col, o);
        continue;
      }
    }
    if (fmt == FMT_GRP) {
      float o[8];
      grp_unpack8(src, a, col, o);
      store8(out + col, o);
      continue;
    }
    if constexpr (ROT) {
      if (fmt == FMT_GRPR) {
        float o[8];
        grp_unpack8_rot(src, a, col, o);
        store8(out + col, o);
        continue;
      }
    }
    int q[8];
    if (fmt == FMT_INT8) {
      const u32x2_t w = *(const u32x2_t*)(src + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[e] = (int)(int8_t)((w[0] >> (8 * e)) & 255);
        q[4 + e] = (int)(int8_t)((w[1] >> (8 * e)) & 255);
      }
    } else if (fmt == FMT_INT4) {
      const uint32_t w = *(const uint32_t*)(src + col / 2);
#pragma unroll
      for (int e = 0; e < 8; ++e) q[e] = ((int)(w << (28 - 4 * e))) >> 28;
    } else {
      const uint32_t w = *(const uint16_t*)(src + col / 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) q[e] = ((int)(w << (30 - 2 * e))) >> 30;
    }
    float o[8];
    if constexpr (RR) {   // x' = H128 q (s / 16); the 16 lanes of the block's DPP row are here (wht_row16)
      if (rrow) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (float)q[e];
        wht_row16(o);
        const float sc = s * 0.0625f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] *= sc;
        store8(out + col, o);
        continue;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float qf = (float)q[e];
      if (a.scale_mode == SC_TOKEN) o[e] = tok_value(qf, s);
      else if (a.scale_mode == SC_WINDOW) o[e] = win_value(qf, qmax, s);
      else {
        const float sc = scales[(size_t)b * a.H + col + e];
        o[e] = (a.ch_kind == CH_MEAN || qmax == 1) ? qf * sc : qf * sc / (float)qmax;
      }
    }
    if constexpr (OUT) {
      if (orow) out_patch(o, op, c);
    }
    store8(out + col, o);
  }
}

// ---------------------------------------------------------------------------------------------
// Fork (the sweep's step between prefix and suffix): one hidden state x [B S, H] in, the receiver-side activations of
// V (importance source, k) variants of ONE codec out, stacked: out[(v B + b) S + j] is what unpack_kernel would write
// for token j of window b from the message pack_kernel builds with the k_v least important tokens of source src_v in
// the lo class - bit for bit, through the same device functions, with no message in between.  Three launches:
//   row_absmax_kernel (SC_WINDOW only): the bits of max|x| of every row, one wave per row.
//   rank_scan_kernel : one workgroup per (source, window) sorts select_sort_kernel's keys once for all k and writes
//                      rank[src][b][j], token j's position in the ascending order: token j is lo in variant v
//                      <=> rank[src_v][b][j] < k_v.  SC_WINDOW: the window scale of variant v, the max|x| over its lo
//                      rows (channel_stats only_lo + rowmax), is the k_v-th inclusive prefix umax of the rows' max-abs
//                      bits along that order (an LDS block scan; maxima of abs_bits patterns: order-independent,
//                      NaN-propagating), 0 for k_v = 0: wscale[v][b].
//   fork_kernel      : one wave per token row loads the row once (load_row8), takes its max-abs once and loops over
//                      the variants: class -> format, qmax, scale (per token from the row max, per window from
//                      wscale) -> codes -> values in registers -> one row store per variant.  Native rows are copied.
// Row formats: the activation dtype's native format, INT8, INT4, INT2; scale modes SC_TOKEN and SC_WINDOW; fixed k.
// The variant table tab[v] = (src_v, k_v) is int32 on the device; V <= FORK_MAXV per launch.
constexpr int FORK_MAXV = 64;
// The fork kernels are compiled without gfx950's packed fp32 instructions (v_pk_mul_f32 and kin): every multiply of a
// row is its own scalar-per-lane instruction.  Device pass only - the host pass has no such feature to switch.
#if defined(__HIP_DEVICE_COMPILE__)
#define FORK_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define FORK_NO_PK_F32
#endif

template <int NCH, class T>
__global__ FORK_NO_PK_F32 __launch_bounds__(256) void row_absmax_kernel(const T* __restrict__ x, uint32_t* __restrict__ amax,
                                                         int rows, int H) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[NCH][8];
  load_row8<NCH>(x + (size_t)row * H, H, v);
  uint32_t amb = 0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) amb = umax(amb, umax8(v[c]));
  amb = wave_umax(amb);
  if ((threadIdx.x & 63) == 0) amax[row] = amb;
}

// grid (sources, B).  imp [nsrc, B, S] (null: one source in position order - every variant has k in {0, S});
// rank [nsrc, B, S]; amax [B, S] row max-abs bits (null unless SC_WINDOW); wscale [V, B].
// LDS: P keys, then S prefix words when amax is given.
__global__ FORK_NO_PK_F32 __launch_bounds__(SEL_T) void rank_scan_kernel(const float* __restrict__ imp, int B, int S, int P,
                                                          int* __restrict__ rank, const uint32_t* __restrict__ amax,
                                                          const int* __restrict__ tab, int V,
                                                          float* __restrict__ wscale) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
  uint32_t* pm = (uint32_t*)(keys + P);
  __shared__ uint32_t part[SEL_T];
  const int src = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t wb = ((size_t)src * B + b) * S;
  for (int i = tid; i < P; i += SEL_T)
    keys[i] = i < S ? (imp ? sel_key(imp[wb + i], i) : (unsigned long long)i) : ~0ull;
  __syncthreads();
  if (imp) bitonic_sort_keys(keys, P);
  for (int p = tid; p < S; p += SEL_T) rank[wb + (int)(keys[p] & 0xFFFFFFFFu)] = p;
  if (!amax) return;
  // inclusive prefix umax of the rows' max-abs bits in sorted order; thread t owns the run [t C, t C + C)
  for (int p = tid; p < S; p += SEL_T) pm[p] = amax[(size_t)b * S + (int)(keys[p] & 0xFFFFFFFFu)];
  __syncthreads();
  const int C = (S + SEL_T - 1) / SEL_T;
  const int i0 = tid * C;
  uint32_t run = 0;
  for (int e = 0; e < C && i0 + e < S; ++e) run = umax(run, pm[i0 + e]);
  part[tid] = run;
  __syncthreads();
  for (int off = 1; off < SEL_T; off <<= 1) {  // Hillis-Steele inclusive scan of the run maxima
    const uint32_t o = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] = umax(part[tid], o);
    __syncthreads();
  }
  uint32_t acc = tid ? part[tid - 1] : 0u;
  for (int e = 0; e < C && i0 + e < S; ++e) {
    acc = umax(acc, pm[i0 + e]);
    pm[i0 + e] = acc;
  }
  __syncthreads();
  for (int v = tid; v < V; v += SEL_T) {
    if (tab[2 * v] != src) continue;
    const int k = min(tab[2 * v + 1], S);
    wscale[(size_t)v * B + b] = k > 0 ? __uint_as_float(pm[k - 1]) : 0.f;
  }
}

struct ForkArgs {
  const void* x; void* out;
  const int* rank;              // [nsrc, B, S]; null: no variant has 0 < k < S
  const float* wscale;          // [V, B] (SC_WINDOW)
  const int* tab;               // [V, 2] (source, k)
  int B, S, H, V;
  int hi_fmt, lo_fmt, scale_mode, qmax_hi, qmax_lo;
};

template <int NCH, class T>
__global__ FORK_NO_PK_F32 __launch_bounds__(256) void fork_kernel(ForkArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.S) return;
  const int lane = threadIdx.x & 63;
  const int b = row / a.S, j = row - b * a.S;
  float v[NCH][8];
  load_row8<NCH>((const T*)a.x + (size_t)row * a.H, a.H, v);
  uint32_t amb = 0;
#pragma unroll
  for (int c = 0; c < NCH; ++c) amb = umax(amb, umax8(v[c]));
  const float am = __uint_as_float(wave_umax(amb));   // NaN / Inf if the row holds one
  const size_t rows = (size_t)a.B * a.S;
  for (int vi = 0; vi < a.V; ++vi) {
    const int src = a.tab[2 * vi], k = a.tab[2 * vi + 1];
    const bool is_lo = a.rank ? a.rank[((size_t)src * a.B + b) * a.S + j] < k : k >= a.S;
    const int fmt = is_lo ? a.lo_fmt : a.hi_fmt, qmax = is_lo ? a.qmax_lo : a.qmax_hi;
    T* out = (T*)a.out + ((size_t)vi * rows + row) * a.H;
    if (fmt == FMT_BF16 || fmt == FMT_F32) {   // native row: the activation's own bits
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int col = (c * 64 + lane) * 8;
        if (col < a.H) store8(out + col, v[c]);
      }
      continue;
    }
    const float qmaxf = (float)qmax, qminf = qmin_of(a.scale_mode, qmax);
    float s, inv = 0.f;
    if (a.scale_mode == SC_TOKEN) {
      s = tok_scale(am, qmax);
      inv = tok_inv(am, s);
    } else {
      s = a.wscale[(size_t)vi * a.B + b];
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = (c * 64 + lane) * 8;
      if (col >= a.H) continue;
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // (float)(int)code: the code as the message carries it
        if (a.scale_mode == SC_TOKEN) o[e] = tok_value((float)(int)tok_code(v[c][e], inv, qmaxf, qminf), s);
        else o[e] = win_value((float)(int)win_code(v[c][e], s, qmaxf, qminf), qmax, s);
      }
      store8(out + col, o);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Measured quantization error of the head groups (codec/plan.py allocate_group_bits_measured): for every window b,
// 64-channel group g, basis (0 plain, 1 Hadamard) and width j of GROUP_BITS,
//   err[b, g, 0, j] = sum_t sum_c dx_tc^2 (x_tc - q_tc s_t)^2,
//   err[b, g, 1, j] = the same of y = H64 x / 8 and dy = H64 dx / 8,
// with q, s exactly grp_pack8's at that width (grp_quant / grp_q) and q s what grp_unpack8 returns; dx == nullptr:
// every weight 1 in both bases.  H64 / 8 is orthonormal and its own inverse, so dy e is the first-order output change
// of the decoded rgroup_rot row as dx e is of the rgroup row.  One wave per token row as in pack_kernel (a lane holds
// 8 consecutive channels of each 512-channel chunk, a group is 8 adjacent lanes); the group's max-abs is taken once
// per basis and shared by the six widths.  q s is rounded to fp32 before the subtraction and the term is
// (dx dx) (e e), one rounding per operation (fp contract off): every term has the bits of the CPU oracle's
// (ops/reference.py group_quant_err), only the order of the sums differs.  A workgroup walks QE_ROWS rows of one window
// (wave w rows w, w + 4, ...), then sums a group's 8 lanes by shuffles and the 4 waves through LDS in a fixed order
// into part[b, chunk, g, 2, 6]; group_quant_err_sum_kernel adds the chunks in order.  No atomics: a rerun is
// bit-identical.
// A group holding a NaN / Inf gets non-finite sums for all twelve entries (s is non-finite, or q s = 0 * Inf); an
// all-zero group adds 0.
constexpr int QE_ROWS = 128;
constexpr int QE_NW = 6;     // widths: GROUP_BITS
template <int QMAX>
__device__ __forceinline__ void qerr_acc8(const float (&v)[8], const float (&w2)[8], float am, float& acc) {
#pragma clang fp contract(off)
  const GrpQuant k = grp_quant(am, QMAX);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float r = grp_q(v[e], k) * k.s;
    const float d = v[e] - r;
    const float t = w2[e] * (d * d);
    acc += t;
  }
}
__device__ __forceinline__ void qerr_widths8(const float (&v)[8], const float (&w)[8], float (&acc)[QE_NW]) {
#pragma clang fp contract(off)
  const float am = __uint_as_float(grp_amax_bits(v));
  float w2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) w2[e] = w[e] * w[e];
  qerr_acc8<1>(v, w2, am, acc[0]);
  qerr_acc8<3>(v, w2, am, acc[1]);
  qerr_acc8<7>(v, w2, am, acc[2]);
  qerr_acc8<15>(v, w2, am, acc[3]);
  qerr_acc8<31>(v, w2, am, acc[4]);
  qerr_acc8<127>(v, w2, am, acc[5]);
}

template <int NCH, class T>
__global__ __launch_bounds__(256) void group_quant_err_kernel(const T* __restrict__ x, const float* __restrict__ dx,
                                                              float* __restrict__ part, int S, int H,
                                                              int chunks) {
  __shared__ float red[4][NCH * 8][2 * QE_NW];
  const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int G = H / 64;
  const int t0 = chunk * QE_ROWS, t1 = min(S, t0 + QE_ROWS);
  float acc[NCH][2][QE_NW];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int k = 0; k < 2 * QE_NW; ++k) acc[c][k / QE_NW][k % QE_NW] = 0.f;
  for (int t = t0 + wave; t < t1; t += 4) {
    const size_t row = (size_t)b * S + t;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c * 512 >= H) continue;            // wave-uniform: whole groups (H % 64 == 0) leave together below too
      float v[1][8], d[1][8];
      load_row8<1>(x + row * H + c * 512, H - c * 512, v);
      if (dx) load_row8<1>(dx + row * H + c * 512, H - c * 512, d);
      else fill8(d[0], 1.f);
      if (c * 512 + lane * 8 >= H) continue;
      qerr_widths8(v[0], d[0], acc[c][0]);
      float y[8], dy[8];
      grp_rotate8(v[0], y);
      if (dx) grp_rotate8(d[0], dy);
      else fill8(dy, 1.f);
      qerr_widths8(y, dy, acc[c][1]);
    }
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int k = 0; k < 2 * QE_NW; ++k) {
      float s = acc[c][k / QE_NW][k % QE_NW];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      if ((lane & 7) == 0) red[wave][c * 8 + (lane >> 3)][k] = s;
    }
  __syncthreads();
  float* out = part + (size_t)blockIdx.x * G * (2 * QE_NW);
  for (int i = threadIdx.x; i < G * 2 * QE_NW; i += 256) {
    const int g = i / (2 * QE_NW), k = i % (2 * QE_NW);
    out[i] = (red[0][g][k] + red[1][g][k]) + (red[2][g][k] + red[3][g][k]);
  }
}

// err[b, i] = sum over the chunks, in order, of part[b, chunk, i]   (i over G x 2 x 6)
__global__ __launch_bounds__(256) void group_quant_err_sum_kernel(const float* __restrict__ part,
                                                                  float* __restrict__ err, int chunks, int n,
                                                                  long long total) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;   // over B x n
  if (j >= total) return;
  const long long b = j / n, i = j - b * n;
  const float* p = part + (size_t)b * chunks * n + i;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += p[(size_t)c * n];
  err[j] = s;
}

#define DISPATCH_NCH(H, ...)                                          \
  do {                                                                \
    const int _nch = ((H) / 8 + 63) / 64;                             \
    if (_nch <= 1) { constexpr int NCH = 1; __VA_ARGS__; }            \
    else if (_nch <= 2) { constexpr int NCH = 2; __VA_ARGS__; }       \
    else if (_nch <= 4) { constexpr int NCH = 4; __VA_ARGS__; }       \
    else if (_nch <= 8) { constexpr int NCH = 8; __VA_ARGS__; }       \
    else return (int)hipErrorInvalidValue;                            \
  } while (0)

static int mask_words(int S) { return ((S + 63) / 64) * 2; }   // per window: whole 64-token pairs of u32

// mode 0: k least important per window; mode 1: top-rho cut at mass thr, k per window -> msg + off_kvec (int32).
EDGE_API int edge_select(const float* imp, int B, int S, int k, void* msg, long long off_mask, int mode, float thr,
                         long long off_kvec, hipStream_t st) {
  if (B <= 0) return 0;
  if (S <= 0 || S > 8192 || (mode == 1 && off_kvec < 0)) return (int)hipErrorInvalidValue;
  int P = 1;
  while (P < S) P <<= 1;
  const int mw = mask_words(S);
  const size_t lds = (size_t)P * 8 + (size_t)mw * 4;
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)select_sort_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(select_sort_kernel, dim3(B), dim3(SEL_T), lds, st, imp, S, P, mode, k, thr,
                     (uint32_t*)((uint8_t*)msg + off_mask), mw, off_kvec >= 0 ? (int*)((uint8_t*)msg + off_kvec) : nullptr);
  return (int)hipGetLastError();
}

// Constant lo-class mask (k = 0 or k = S): a kernel, not hipMemsetAsync - inside a captured HIP graph the memset node
// was measured to lose its order against the message's zero fill (replays produced an all-zero mask for k = S).
// k = S sets the bits of the S tokens only - bit j <=> token j, as select_sort_kernel and the CPU codec write it: the
// padding bits of a partial last word (S % 64 != 0) stay 0, so the message is the CPU's byte for byte.
__global__ __launch_bounds__(256) void set_mask_kernel(uint32_t* __restrict__ mask, size_t nwords, int mw, int S,
                                                       int all_lo) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nwords) return;
  const int n = S - 32 * (int)(i % (size_t)mw);   // tokens from this word's bit 0 on
  mask[i] = !all_lo || n <= 0 ? 0u : n >= 32 ? 0xffffffffu : (1u << n) - 1u;
}

EDGE_API int edge_set_mask(void* msg, long long off_mask, int B, int S, int all_lo, hipStream_t st) {
  const int mw = mask_words(S);
  const size_t n = (size_t)B * mw;
  if (!n) return 0;
  if (off_mask % 4) return (int)hipErrorInvalidValue;
  set_mask_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>((uint32_t*)((uint8_t*)msg + off_mask), n, mw, S,
                                                                all_lo);
  return (int)hipGetLastError();
}

// channel_stats: mode 0 max|x|, 1 mean+1e-8; only_lo restricts to lo-class rows.  out: [B, H] fp32
EDGE_API int edge_channel_stats(const void* x, const void* msg, long long off_mask, float* out, int B, int S, int H,
                                int mode, int only_lo, int x_f32, hipStream_t st) {
  if (B <= 0) return 0;
  const int mw = mask_words(S);
  const uint32_t* mask = (const uint32_t*)((const uint8_t*)msg + off_mask);
  if (x_f32)
    hipLaunchKernelGGL(channel_stats_kernel<float>, dim3(B, (H + 63) / 64), dim3(256), 0, st, (const float*)x, mask,
                       mw, out, S, H, mode, only_lo);
  else
    hipLaunchKernelGGL(channel_stats_kernel<bf16_t>, dim3(B, (H + 63) / 64), dim3(256), 0, st, (const bf16_t*)x, mask,
                       mw, out, S, H, mode, only_lo);
  return (int)hipGetLastError();
}

EDGE_API int edge_rowmax(const float* in, float* out, int R, int H, hipStream_t st) {
  if (R <= 0) return 0;
  rowmax_kernel<<<R, 256, 0, st>>>(in, out, H);
  return (int)hipGetLastError();
}

// grp_code_bytes: FMT_GRP / FMT_GRPR rows' code bytes (sum 8 b_g over the plan at msg + opl; 0 without such rows).
// A message with FMT_GRPR rows goes to the ROT instantiations (which handle every other format too).
static bool has_fmt(int hi_fmt, int lo_fmt, int fmt) { return hi_fmt == fmt || lo_fmt == fmt; }

template <bool PACK, int NCH, class T, bool ROT, bool W16 = false, bool MX6 = false, bool MXR = false, bool OUT = false,
          bool RR = false, bool RF = false, bool NV4 = false>
static void launch_codec(dim3 grid, hipStream_t st, const CodecArgs& a) {
  if constexpr (PACK)
    hipLaunchKernelGGL((pack_kernel<NCH, T, ROT, W16, MX6, MXR, OUT, RR, RF, NV4>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((unpack_kernel<NCH, T, ROT, W16, MX6, MXR, OUT, RR, RF, NV4>), grid, dim3(256), 0, st, a);
}

// edge_pack / edge_unpack: argument checks, CodecArgs and the (ROT | W16 | plain) x activation dtype x NCH dispatch.
// A message with FMT_F16 / FMT_F16S rows goes to the W16 instantiations (which handle every format but FMT_GRPR);
// together with FMT_GRPR rows it is rejected before anything is launched.  A message with FMT_MXFP6 / FMT_MXBF6 rows goes
// to the MX6 instantiations; together with FMT_GRPR, FMT_F16 or FMT_F16S rows it is rejected the same way.  A message
// with rotated MX rows goes to the MXR instantiations - MXR x MX6 when one of them is 6-bit - under the same rejections.
// A message with outlier rows goes to the OUT instantiations; with any scale mode but SC_TOKEN, or next to head-group,
// 16-bit, 6-bit or rotated rows, it is rejected before anything is launched.  A message with rotated int rows goes to the
// RR instantiations; with H % 128 != 0, any scale mode but SC_TOKEN, or next to head-group, 16-bit, 6-bit, rotated MX or
// outlier rows, it is rejected the same way.  A message with row-rotated int rows goes to the RF instantiations; with a
// hidden size that is neither 2^7 .. 2^12 nor 28 * 2^5 .. 28 * 2^7, any scale mode but SC_TOKEN, or next to head-group,
// 16-bit, 6-bit, rotated MX, outlier or block-rotated (h128) rows, it is rejected the same way.  A message with NVFP4
// rows goes to the NV4 instantiations; next to head-group, 16-bit, 6-bit, rotated MX, outlier, h128 or row-rotated rows
// it is rejected the same way.
template <bool PACK>
static int run_codec(void* x, void* msg, long long om, long long os, long long oh, long long ol, long long okv,
                     long long opl, int B, int S, int H, int k, int hi_fmt, int lo_fmt, int scale_mode, int qmax_hi,
                     int qmax_lo, int ch_kind, int grp_code_bytes, int x_f32, hipStream_t st) {
  if (H % 32) return (int)hipErrorInvalidValue;
  const bool rot = has_fmt(hi_fmt, lo_fmt, FMT_GRPR);
  const bool w16 = has_fmt(hi_fmt, lo_fmt, FMT_F16) || has_fmt(hi_fmt, lo_fmt, FMT_F16S);
  const bool mxr6 = has_fmt(hi_fmt, lo_fmt, FMT_MXFP6R) || has_fmt(hi_fmt, lo_fmt, FMT_MXBF6R);
  const bool mxr = mxr6 || has_fmt(hi_fmt, lo_fmt, FMT_MXFP4R) || has_fmt(hi_fmt, lo_fmt, FMT_MXFP8R);
  const bool mx6 = mxr6 || has_fmt(hi_fmt, lo_fmt, FMT_MXFP6) || has_fmt(hi_fmt, lo_fmt, FMT_MXBF6);
  const bool out = has_fmt(hi_fmt, lo_fmt, FMT_INT8O) || has_fmt(hi_fmt, lo_fmt, FMT_INT4O) ||
                   has_fmt(hi_fmt, lo_fmt, FMT_INT2O);
  const bool rr = has_fmt(hi_fmt, lo_fmt, FMT_INT8R) || has_fmt(hi_fmt, lo_fmt, FMT_INT4R) ||
                  has_fmt(hi_fmt, lo_fmt, FMT_INT2R);
  if ((rot && w16) || ((mx6 || mxr) && (rot || w16))) return (int)hipErrorInvalidValue;
  if (out && (rot || w16 || mx6 || mxr || has_fmt(hi_fmt, lo_fmt, FMT_GRP) || scale_mode != SC_TOKEN))
    return (int)hipErrorInvalidValue;
  if (rr && (out || rot || w16 || mx6 || mxr || has_fmt(hi_fmt, lo_fmt, FMT_GRP) || scale_mode != SC_TOKEN || H % 128))
    return (int)hipErrorInvalidValue;
  const bool rf = has_fmt(hi_fmt, lo_fmt, FMT_INT8F) || has_fmt(hi_fmt, lo_fmt, FMT_INT4F) ||
                  has_fmt(hi_fmt, lo_fmt, FMT_INT2F);
  if (rf && (rr || out || rot || w16 || mx6 || mxr || has_fmt(hi_fmt, lo_fmt, FMT_GRP) || scale_mode != SC_TOKEN ||
             !rf_size_ok(H)))
    return (int)hipErrorInvalidValue;
  const bool nv4 = has_fmt(hi_fmt, lo_fmt, FMT_NVFP4);
  if (nv4 && (rf || rr || out || rot || w16 || mx6 || mxr || has_fmt(hi_fmt, lo_fmt, FMT_GRP)))
    return (int)hipErrorInvalidValue;
  if ((rot || has_fmt(hi_fmt, lo_fmt, FMT_GRP)) && (H % 64 || opl < 0 || grp_code_bytes <= 0))
    return (int)hipErrorInvalidValue;
  CodecArgs a;
  a.x = x; a.msg = (uint8_t*)msg;
  a.off_mask = om; a.off_scale = os; a.off_hi = oh; a.off_lo = ol; a.off_kvec = okv; a.off_plan = opl;
  a.grp_code_bytes = grp_code_bytes;
  a.B = B; a.S = S; a.H = H; a.k = k; a.mw = mask_words(S);
  a.hi_fmt = hi_fmt; a.lo_fmt = lo_fmt; a.scale_mode = scale_mode; a.qmax_hi = qmax_hi; a.qmax_lo = qmax_lo;
  a.ch_kind = ch_kind;
  const int rows = B * S;
  if (rows <= 0) return 0;
  const dim3 grid((rows + 3) / 4);
  if (rot && x_f32) DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, true>(grid, st, a)));
  else if (rot) DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, true>(grid, st, a)));
  else if (w16 && x_f32) DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false, true>(grid, st, a)));
  else if (w16) DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false, true>(grid, st, a)));
  else if (mxr && mx6 && x_f32) DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false, false, true, true>(grid, st, a)));
  else if (mxr && mx6) DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false, false, true, true>(grid, st, a)));
  else if (mxr && x_f32) DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false, false, false, true>(grid, st, a)));
  else if (mxr) DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false, false, false, true>(grid, st, a)));
  else if (mx6 && x_f32) DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false, false, true>(grid, st, a)));
  else if (mx6) DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false, false, true>(grid, st, a)));
  else if (out && x_f32) DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false, false, false, false, true>(grid, st, a)));
  else if (out) DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false, false, false, false, true>(grid, st, a)));
  else if (rr && x_f32)
    DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false, false, false, false, false, true>(grid, st, a)));
  else if (rr) DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false, false, false, false, false, true>(grid, st, a)));
  else if (rf && x_f32)
    DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false, false, false, false, false, false, true>(grid, st, a)));
  else if (rf)
    DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false, false, false, false, false, false, true>(grid, st, a)));
  else if (nv4 && x_f32)
    DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false, false, false, false, false, false, false, true>(grid, st, a)));
  else if (nv4)
    DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false, false, false, false, false, false, false, true>(grid, st, a)));
  else if (x_f32) DISPATCH_NCH(H, (launch_codec<PACK, NCH, float, false>(grid, st, a)));
  else DISPATCH_NCH(H, (launch_codec<PACK, NCH, bf16_t, false>(grid, st, a)));
  return (int)hipGetLastError();
}

EDGE_API int edge_pack(const void* x, void* msg, long long om, long long os, long long oh, long long ol, long long okv,
                       long long opl, int B, int S, int H, int k, int hi_fmt, int lo_fmt, int scale_mode, int qmax_hi,
                       int qmax_lo, int ch_kind, int grp_code_bytes, int x_f32, hipStream_t st) {
  return run_codec<true>((void*)x, msg, om, os, oh, ol, okv, opl, B, S, H, k, hi_fmt, lo_fmt, scale_mode, qmax_hi,
                         qmax_lo, ch_kind, grp_code_bytes, x_f32, st);
}

EDGE_API int edge_unpack(void* x, const void* msg, long long om, long long os, long long oh, long long ol,
                         long long okv, long long opl, int B, int S, int H, int k, int hi_fmt, int lo_fmt,
                         int scale_mode, int qmax_hi, int qmax_lo, int ch_kind, int grp_code_bytes, int x_f32,
                         hipStream_t st) {
  return run_codec<false>(x, (void*)msg, om, os, oh, ol, okv, opl, B, S, H, k, hi_fmt, lo_fmt, scale_mode, qmax_hi,
                          qmax_lo, ch_kind, grp_code_bytes, x_f32, st);
}

// err [B, H/64, 2, 6] fp32; ws: edge_group_quant_err_chunks(S) * B * H/64 * 12 floats; dx fp32 or null (weights 1)
EDGE_API int edge_group_quant_err_chunks(int S) { return (S + QE_ROWS - 1) / QE_ROWS; }

template <int NCH, class T>
static void launch_qerr(dim3 grid, hipStream_t st, const void* x, const float* dx, float* ws, int S, int H,
                        int chunks) {
  hipLaunchKernelGGL((group_quant_err_kernel<NCH, T>), grid, dim3(256), 0, st, (const T*)x, dx, ws, S, H, chunks);
}

EDGE_API int edge_group_quant_err(const void* x, const float* dx, float* err, float* ws, int B, int S, int H,
                                  int x_is_f32, hipStream_t st) {
  if (H <= 0 || H % 64 || B < 0 || S <= 0) return (int)hipErrorInvalidValue;
  const int chunks = edge_group_quant_err_chunks(S);
  if ((long long)B * chunks > 0x7fffffffll) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)(B * chunks));
  if (B == 0) { DISPATCH_NCH(H, (void)0); return 0; }   // a bad H is an error whatever B
  if (x_is_f32) DISPATCH_NCH(H, (launch_qerr<NCH, float>(grid, st, x, dx, ws, S, H, chunks)));
  else DISPATCH_NCH(H, (launch_qerr<NCH, bf16_t>(grid, st, x, dx, ws, S, H, chunks)));
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  const int n = H / 64 * 2 * QE_NW;
  const long long total = (long long)B * n;
  group_quant_err_sum_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(ws, err, chunks, n, total);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// edge_fake_quant_fork: x [B S, H] -> out [V B S, H] (the activation dtype), see fork_kernel.  imp [nsrc, B, S] fp32
// (nsrc = 0: null, every k in {0, S}); tab [V, 2] int32 on the device with 0 <= source < max(nsrc, 1); workspaces
// rank [max(nsrc, 1) B S] int32, amax [B S] u32 and wscale [V B] fp32 (the last two for SC_WINDOW only).
template <int NCH, class T>
static void launch_fork(dim3 grid, hipStream_t st, const ForkArgs& a, uint32_t* amax) {
  if (amax) hipLaunchKernelGGL((row_absmax_kernel<NCH, T>), grid, dim3(256), 0, st, (const T*)a.x, amax, a.B * a.S, a.H);
  else hipLaunchKernelGGL((fork_kernel<NCH, T>), grid, dim3(256), 0, st, a);
}

static bool fork_fmt_ok(int fmt, int qmax, int native) {
  return fmt == native || (fmt == FMT_INT8 && qmax == 127) || (fmt == FMT_INT4 && qmax == 7) ||
         (fmt == FMT_INT2 && qmax == 1);
}

EDGE_API int edge_fake_quant_fork(const void* x, void* out, const float* imp, int nsrc, const int* tab, int V,
                                  int* rank, void* amax, float* wscale, int B, int S, int H, int hi_fmt, int lo_fmt,
                                  int scale_mode, int qmax_hi, int qmax_lo, int x_f32, hipStream_t st) {
  const int native = x_f32 ? FMT_F32 : FMT_BF16;
  if (H <= 0 || H % 32 || S <= 0 || S > 8192 || B < 0 || V <= 0 || V > FORK_MAXV || nsrc < 0 || (nsrc > 0 && !imp) ||
      (scale_mode != SC_TOKEN && scale_mode != SC_WINDOW) || !fork_fmt_ok(hi_fmt, qmax_hi, native) ||
      !fork_fmt_ok(lo_fmt, qmax_lo, native) || (long long)B * S > 0x7fffffffll)
    return (int)hipErrorInvalidValue;
  const bool window = scale_mode == SC_WINDOW;
  if (window && (!amax || !wscale)) return (int)hipErrorInvalidValue;
  if ((nsrc > 0 || window) && !rank) return (int)hipErrorInvalidValue;
  ForkArgs a;
  a.x = x; a.out = out; a.rank = nsrc > 0 || window ? rank : nullptr; a.wscale = wscale; a.tab = tab;
  a.B = B; a.S = S; a.H = H; a.V = V;
  a.hi_fmt = hi_fmt; a.lo_fmt = lo_fmt; a.scale_mode = scale_mode; a.qmax_hi = qmax_hi; a.qmax_lo = qmax_lo;
  if (B == 0) { DISPATCH_NCH(H, (void)0); return 0; }
  const dim3 grid((unsigned)(((long long)B * S + 3) / 4));
  if (window) {
    if (x_f32) DISPATCH_NCH(H, (launch_fork<NCH, float>(grid, st, a, (uint32_t*)amax)));
    else DISPATCH_NCH(H, (launch_fork<NCH, bf16_t>(grid, st, a, (uint32_t*)amax)));
  }
  if (a.rank) {
    int P = 1;
    while (P < S) P <<= 1;
    const size_t lds = (size_t)P * 8 + (window ? (size_t)S * 4 : 0);
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)rank_scan_kernel,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(rank_scan_kernel, dim3(nsrc > 0 ? nsrc : 1, B), dim3(SEL_T), lds, st, imp, B, S, P, rank,
                       window ? (const uint32_t*)amax : nullptr, tab, V, wscale);
  }
  if (x_f32) DISPATCH_NCH(H, (launch_fork<NCH, float>(grid, st, a, nullptr)));
  else DISPATCH_NCH(H, (launch_fork<NCH, bf16_t>(grid, st, a, nullptr)));
  return (int)hipGetLastError();
}
