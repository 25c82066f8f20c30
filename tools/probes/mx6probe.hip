// What gfx950's fp6 scaled converts do (hipcc --offload-arch=gfx950 -O2 mx6probe.hip -o mx6probe): where the two
// 16-float operands of v_cvt_scalef32_2xpk16_{fp6,bf6}_f32 land in the six dwords ("slot" c = bits [6 c, 6 c + 6):
// operand 0's element p is slot 2 p, operand 1's slot 2 p + 1), ties, saturation, the sign of zeros, denormal scales
// and inputs, and what v_cvt_scalef32_pk32_f32_{fp6,bf6} returns for the natural stream of codes.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
typedef __attribute__((ext_vector_type(16))) float f16v;
typedef __attribute__((ext_vector_type(32))) float f32v;
typedef __attribute__((ext_vector_type(6))) unsigned u6v;
// in: 32 floats, scale.  out: 6 dwords fp6, 6 dwords bf6 (in0 = first 16, in1 = last 16), then decode of both
__global__ void enc(const float* x, float scale, unsigned* o, float* r) {
  if (threadIdx.x) return;
  f16v a, b;
  for (int i = 0; i < 16; ++i) { a[i] = x[i]; b[i] = x[16 + i]; }
  u6v p = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, scale);
  u6v q = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, scale);
  for (int i = 0; i < 6; ++i) { o[i] = p[i]; o[6 + i] = q[i]; }
  f32v d = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(p, scale);
  f32v e = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(q, scale);
  for (int i = 0; i < 32; ++i) { r[i] = d[i]; r[32 + i] = e[i]; }
}
// decode of the natural stream: code c at bits [6c, 6c+6), c = 0..31 then 32..63 -> 64 floats each type
__global__ void dec(const unsigned* s, float scale, float* r) {
  if (threadIdx.x) return;
  for (int h = 0; h < 2; ++h) {
    u6v p;
    for (int i = 0; i < 6; ++i) p[i] = s[6 * h + i];
    f32v d = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(p, scale);
    f32v e = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(p, scale);
    for (int i = 0; i < 32; ++i) { r[32 * h + i] = d[i]; r[64 + 32 * h + i] = e[i]; }
  }
}
static unsigned code_at(const unsigned* w, int c) {
  unsigned long long v = 0;
  int bit = 6 * c, d = bit >> 5, sh = bit & 31;
  v = w[d];
  if (d + 1 < 6) v |= (unsigned long long)w[d + 1] << 32;
  return (unsigned)(v >> sh) & 63u;
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
int main() {
  float *dx, *dr; unsigned *dout, *ds;
  CK(hipMalloc(&dx, 32 * 4)); CK(hipMalloc(&dr, 128 * 4)); CK(hipMalloc(&dout, 12 * 4)); CK(hipMalloc(&ds, 12 * 4));
  float hx[32], hr[128]; unsigned ho[12];
  auto run = [&](const char* name, float scale) -> int {
    CK(hipMemcpy(dx, hx, 128, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(enc, 1, 64, 0, 0, dx, scale, dout, dr);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(ho, dout, 48, hipMemcpyDeviceToHost)); CK(hipMemcpy(hr, dr, 256, hipMemcpyDeviceToHost));
    unsigned sb; memcpy(&sb, &scale, 4);
    printf("== %s scale bits %08x\n fp6 dwords:", name, sb);
    for (int i = 0; i < 6; ++i) printf(" %08x", ho[i]);
    printf("\n bf6 dwords:");
    for (int i = 0; i < 6; ++i) printf(" %08x", ho[6 + i]);
    printf("\n");
    for (int i = 0; i < 32; ++i) {
      unsigned xb, r0, r1; memcpy(&xb, &hx[i], 4); memcpy(&r0, &hr[i], 4); memcpy(&r1, &hr[32 + i], 4);
      printf("  i=%2d x=%14.6g (%08x) fp6 slot=%02x rt=%14.6g (%08x) | bf6 slot=%02x rt=%14.6g (%08x)\n", i, hx[i], xb,
             code_at(ho, i), hr[i], r0, code_at(ho + 6, i), hr[32 + i], r1);
    }
    return 0;
  };
  // 1: distinct values: e2m3 grid points i -> which slot does input i land in
  for (int i = 0; i < 32; ++i) hx[i] = i < 8 ? i * 0.125f : (1.f + (i & 7) * 0.125f) * (float)(1 << ((i >> 3) - 1));
  if (run("e2m3 grid", 1.f)) return 1;
  // 2: e3m2 grid
  for (int i = 0; i < 32; ++i) hx[i] = i < 4 ? i * 0.0625f : (1.f + (i & 3) * 0.25f) * 0.25f * (float)(1 << ((i >> 2) - 1));
  if (run("e3m2 grid", 1.f)) return 1;
  // 3: ties, signs, saturation, NaN/Inf
  {
    const float t[32] = {0.0625f, 0.1875f, 0.3125f, -0.0625f, -0.1875f, 1.0625f, 1.1875f, 7.25f, 7.5f, 7.75f, 7.99f, 8.f,
                         100.f, -7.75f, -100.f, 28.f, 29.f, 30.f, 31.9f, 32.f, -30.f, 26.f, 0.03125f, 0.09375f, -0.f, 0.f,
                         1e30f, __builtin_nanf(""), __builtin_inff(), -__builtin_inff(), 3.25f, 3.75f};
    memcpy(hx, t, 128);
    if (run("ties/sat", 1.f)) return 1;
    if (run("ties/sat scale 4", 4.f)) return 1;
    float s; unsigned b = 0x40e00000u; memcpy(&s, &b, 4);   // 7.0: only the exponent should count (-> 4)
    if (run("ties/sat scale 7.0 (mantissa ignored?)", s)) return 1;
  }
  // 4: denormal scale (E8M0 byte 0 as the codec passes it) with denormal inputs
  {
    float s; unsigned b = 0x00400000u; memcpy(&s, &b, 4);
    for (int i = 0; i < 32; ++i) { unsigned u = (unsigned)i << 18; memcpy(&hx[i], &u, 4); }   // i * 2^-131 .. : i/8 * 2^-128?
    if (run("denormal scale 2^-127, denormal x = i * 2^-131", s)) return 1;
    b = 0x7f000000u; memcpy(&s, &b, 4);   // 2^127
    for (int i = 0; i < 32; ++i) hx[i] = (i - 16) * 0.25f * 1.7014118e38f * 0.5f;
    if (run("scale 2^127", s)) return 1;
  }
  // 5: decode of the natural stream of codes 0..63
  {
    unsigned hs[12] = {0};
    for (int c = 0; c < 64; ++c) {
      const int h = c >> 5, bit = 6 * (c & 31);
      unsigned long long v = (unsigned long long)(c & 63) << (bit & 31);
      hs[6 * h + (bit >> 5)] |= (unsigned)v;
      if ((bit >> 5) + 1 < 6) hs[6 * h + (bit >> 5) + 1] |= (unsigned)(v >> 32);
    }
    CK(hipMemcpy(ds, hs, 48, hipMemcpyHostToDevice));
    const unsigned sc_bits[4] = {0x3f800000u, 0x00400000u, 0x7f800000u, 0x7fc00000u};
    for (unsigned b : sc_bits) {
      float s; memcpy(&s, &b, 4);
      hipLaunchKernelGGL(dec, 1, 64, 0, 0, ds, s, dr);
      CK(hipDeviceSynchronize());
      CK(hipMemcpy(hr, dr, 512, hipMemcpyDeviceToHost));
      printf("== decode natural stream, scale bits %08x\n", b);
      for (int c = 0; c < 64; ++c) {
        unsigned r0, r1; memcpy(&r0, &hr[c], 4); memcpy(&r1, &hr[64 + c], 4);
        printf("  code %2d fp6 %14.6g (%08x) bf6 %14.6g (%08x)\n", c, hr[c], r0, hr[64 + c], r1);
      }
    }
  }
  return 0;
}
