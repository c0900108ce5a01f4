// Device-side building blocks of the conv tile kernels (conv.hip, trunk.hip, resblock.hip and
// the other MFMA kernels): the operand fragment and its relu, the tile geometry and K-chunk tap
// rule (also the host's LDS sizing), the e4m3 conversions, the pixel-index split, the halo'd-tile
// window offset, the relu-gate / residual epilogue steps, the weight-fragment load, the dgrad /
// forward MFMA block, the weight-gradient K block and the stage-0 bit-plane row pieces. Every
// helper is a forced inline of the code its callers used to write out, so the emitted
// instructions are the callers' own.
#pragma once
#include "common.h"

namespace mbk {

// one MFMA A / B operand (v_mfma_f32_16x16x32_bf16): 8 bf16 per lane, as a 16-byte load (u) or
// two transposed LDS reads (h)
union Frag8 {
  bf16x8 v;
  uint4 u;
  s16x4 h[2];
};

__device__ __forceinline__ uint4 relu8(uint4 v) {
  return make_uint4(relu2(v.x), relu2(v.y), relu2(v.z), relu2(v.w));
}
// relu8 by sign-bit tests (v_cmp / v_cndmask per half) instead of v_pk_max_i16: the form that
// fc.hip, pixconv.hip and the trunk's fused head were written and timed with. relu8 gives a
// different (shorter) instruction stream at every one of their call sites, so swapping it in
// is a performance change to measure on its own, not a rename.
__device__ __forceinline__ uint4 relu8_sel(uint4 v) {
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    w[j] = ((w[j] & 0x8000u) ? 0u : (w[j] & 0xFFFFu)) |
           ((w[j] & 0x80000000u) ? 0u : (w[j] & 0xFFFF0000u));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// ------------------------------------------------------------------ tile geometry
// A conv's K = 9 taps x C input channels runs in NCH chunks of 32 (C 32: one tap per chunk; C 16:
// a tap pair, the tenth tap a zero pad); LDS tiles are NHWC with PIXB bytes per bf16 pixel (16
// pad bytes: bank spread) or PIXB8 per e4m3 pixel. Host code sizes LDS by the same numbers.
__host__ __device__ constexpr int conv_nch(int c) { return c == 16 ? 5 : 9; }
__host__ __device__ constexpr int tile_pixb(int c, bool fp8 = false) {
  return fp8 ? c + 8 : c * 2 + 16;
}
template <int C>
struct Geo {
  static constexpr int NCH = conv_nch(C);
  static constexpr int PIXB = tile_pixb(C);
  static constexpr int PIXB8 = tile_pixb(C, true);
};

// The 8 K elements 8g .. 8g+7 of chunk c (an MFMA lane group's fragment): their tap and first
// input channel. Element k of the chunk is chunk_tap(cin, c, k / 8) with channel ch0 + k % 8.
struct ChunkTap {
  int tap, ch0;
};
__host__ __device__ constexpr ChunkTap chunk_tap(int cin, int c, int g) {
  return cin == 16 ? ChunkTap{2 * c + (g >> 1), 8 * (g & 1)} : ChunkTap{c, 8 * g};
}
// ... and their byte offset from the window's tap (0, 0) in a tile of rowpix pixels per row,
// pixb bytes per pixel and eb bytes per element. The pad tap reads tap 8: finite values against
// zero packed weights add exactly 0.
__host__ __device__ constexpr int chunk_off(int cin, int c, int g, int rowpix, int pixb, int eb) {
  const ChunkTap t = chunk_tap(cin, c, g);
  const int tapc = t.tap < 9 ? t.tap : 8;
  return ((tapc / 3) * rowpix + (tapc % 3)) * pixb + t.ch0 * eb;
}

// ------------------------------------------------------------------ fp8 (OCP e4m3) conversion
// 4 floats -> 4 e4m3 bytes, round-to-nearest-even, saturated to +-448
__device__ __forceinline__ uint32_t fp8x4(float a, float b, float c, float d) {
  auto sat = [](float v) { return fminf(fmaxf(v, -448.f), 448.f); };
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(sat(a), sat(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(sat(c), sat(d), w, true);
  return (uint32_t)w;
}
// 4 bf16 (two packed words) -> e4m3, optionally through relu
__device__ __forceinline__ uint32_t bf16x4_fp8(uint2 o, bool relu) {
  if (relu) o = make_uint2(relu2(o.x), relu2(o.y));
  return fp8x4(lo_f(o.x), hi_f(o.x), lo_f(o.y), hi_f(o.y));
}
__device__ __forceinline__ uint2 bf16x8_to_fp8(uint4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  float f[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = lo_f(w[j]);
    f[2 * j + 1] = hi_f(w[j]);
  }
  return make_uint2(fp8x4(f[0], f[1], f[2], f[3]), fp8x4(f[4], f[5], f[6], f[7]));
}

// The kernels map a tile-local pixel index p in [0, imgs*H*W) to (image, y, x) with float
// reciprocals ((p + 0.5) * (1/HW)): exact while imgs*H*W < 2^22 (the product's rounding
// error stays below the 0.5/HW distance to the next integer); the integer divisions by runtime
// H*W / W are ~20 VALU per block. LDS capacity keeps today's shapes far below the bound; the
// launchers check it (launch.h index_math_ok), which turns a future larger-tile / larger-map
// config into a launch error instead of silently wrong indices.
struct Pix {
  int im, y, x;
};
struct PixSplit {
  int HW, W;
  float inv_hw, inv_w;  // 1 / HW, 1 / W
  __device__ __forceinline__ Pix operator()(int p) const {
    const int im = (int)(((float)p + 0.5f) * inv_hw), r = p - im * HW;
    const int y = (int)(((float)r + 0.5f) * inv_w), x = r - y * W;
    return {im, y, x};
  }
};

// A halo'd LDS tile of imgs images: the 3x3 window of pixel (y, x) of image im starts (tap
// (0, 0)) at byte im * imgb + y * rowb + x * pb; the pixel itself is one row and one pixel on
struct TileMap {
  PixSplit split;
  int pb, rowb, imgb;
  __device__ __forceinline__ int win(int p) const {  // window of tile-local pixel p
    const Pix q = split(p);
    return q.im * imgb + q.y * rowb + q.x * pb;
  }
  __device__ __forceinline__ int pixel(int p) const {  // tile-local pixel p itself
    const Pix q = split(p);
    return q.im * imgb + (q.y + 1) * rowb + (q.x + 1) * pb;
  }
  __device__ __forceinline__ int tap(int t) const { return (t / 3) * rowb + (t % 3) * pb; }
};

// ------------------------------------------------------------------ epilogue steps
// relu gate: v[i] = acc[i] where the bf16 mask value i of the two words m is > 0, else 0;
// ADD: + the bf16 value i of the two words a (the residual's gradient)
template <bool ADD>
__device__ __forceinline__ void relu_gate4(f32x4 acc, uint2 m, uint2 a, float (&v)[4]) {
  const uint32_t mw[2] = {m.x, m.y}, aw[2] = {a.x, a.y};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t hb = (mw[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    v[i] = (__uint_as_float(hb << 16) > 0.f) ? acc[i] : 0.f;
    if (ADD) v[i] += __uint_as_float(((aw[i >> 1] >> (16 * (i & 1))) & 0xFFFFu) << 16);
  }
}
__device__ __forceinline__ void relu_gate4(f32x4 acc, uint2 m, float (&v)[4]) {
  relu_gate4<false>(acc, m, m, v);
}
__device__ __forceinline__ void relu_gate_add4(f32x4 acc, uint2 m, uint2 a, float (&v)[4]) {
  relu_gate4<true>(acc, m, a, v);
}
// v[i] += bf16 value i of the two words a (the forward residual add)
__device__ __forceinline__ void add_bf16x4(float (&v)[4], uint2 a) {
  v[0] += lo_f(a.x); v[1] += hi_f(a.x); v[2] += lo_f(a.y); v[3] += hi_f(a.y);
}

// ------------------------------------------------------------------ MFMA blocks
// A fragments of packed conv weights [rows][NCH][32] (conv.hip packed_fwd / packed_bwd): lane
// (g, li) holds row nb * 16 + li, chunk c, elements 8g .. 8g+7
template <int NCH, int NB>
__device__ __forceinline__ void load_wfrags(Frag8 (&w)[NCH][NB], const bf16* wt, int li, int g) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const uint4* wp = (const uint4*)(wt + (size_t)(nb * 16 + li) * NCH * 32 + g * 8);
#pragma unroll
    for (int c = 0; c < NCH; ++c) w[c][nb].u = wp[c * 4];
  }
}

// One 16-pixel block of a 3x3 conv (forward, or dgrad on the transposed weights): NCH tap
// reads at bp + coff[c] (relu'd on the way where the tile holds raw values), each feeding the
// MFMA chains of NB 16-channel output blocks
template <int NCH, int NB>
__device__ __forceinline__ void conv_block16(f32x4 (&acc)[NB], const Frag8 (&w)[NCH][NB],
                                             const char* bp, const int (&coff)[NCH], bool relu) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    Frag8 av;
    av.u = *(const uint4*)(bp + coff[c]);
    if (relu) av.u = relu8(av.u);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[c][nb].v, av.v, acc[nb], 0, 0, 0);
  }
}

// Weight-gradient K block kb (32 pixels of the M in the tiles) of one 16 x 16 channel tile:
// A = dY from tile D (the pixels themselves), B = the nine X taps from tile X, both by
// transposed reads; acc[t] += per tap. D and X point at the tile's first channel of the
// caller's 16-channel block. Out-of-range pixels read `zero` as dY against pixel 0's (finite)
// X values, so they add exactly nothing and need no per-tap select.
__device__ __forceinline__ void wgrad_kblock(f32x4 (&acc)[9], const TileMap& T, int kb, int M,
                                             const char* D, const char* X, const char* zero) {
  const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
  const char* dptr[2];
  int xpos[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int p = kb * 32 + 8 * g + 4 * h + (li >> 2);
    const bool ok = p < M;
    xpos[h] = T.win(ok ? p : 0);
    dptr[h] = ok ? D + xpos[h] + T.rowb + T.pb : zero;
  }
  Frag8 af;
#pragma unroll
  for (int h = 0; h < 2; ++h) af.h[h] = tr_read(dptr[h] + (4 * (li & 3)) * 2);
  const char* xb0 = X + xpos[0] + 8 * (li & 3);
  const char* xb1 = X + xpos[1] + 8 * (li & 3);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    Frag8 bf;
    bf.h[0] = tr_read(xb0 + T.tap(t));
    bf.h[1] = tr_read(xb1 + T.tap(t));
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af.v, bf.v, acc[t], 0, 0, 0);
  }
}

// ------------------------------------------------------------------ stage-0 bit-plane rows
// 8 one-hot planes (the low byte of bits) -> 8 bf16 (1.0 / 0.0): one entry of the stage-0
// conv's byte -> fragment lookup table
__device__ __forceinline__ uint4 bits8_bf16(uint32_t bits) {
  uint32_t w4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    w4[j] = (((bits >> (2 * j)) & 1u) ? 0x3F80u : 0u) |
            (((bits >> (2 * j + 1)) & 1u) ? 0x3F800000u : 0u);
  return make_uint4(w4[0], w4[1], w4[2], w4[3]);
}

// lane x <- lane x-1 / x+1 inside each 16-lane DPP row, zero at the row ends (the stage-0
// conv's zero padding for its kx = 0 / 2 taps)
__device__ __forceinline__ uint32_t dpp_shr1_zero(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x111, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t dpp_shl1_zero(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x101, 0xF, 0xF, true);
}
// the same for floats with -inf at the row ends (max-pool padding)
__device__ __forceinline__ float dpp_shr1_ninf(float v) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp((int)0xFF800000u, __float_as_int(v), 0x111, 0xF, 0xF, false));
}
__device__ __forceinline__ float dpp_shl1_ninf(float v) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp((int)0xFF800000u, __float_as_int(v), 0x101, 0xF, 0xF, false));
}

// One input row of a 16-pixel block of a bit-plane map, lane x holding pixel x's word: the LUT
// byte offsets of pixels x-1 (l), x (c), x+1 (h) for the lane's plane byte
struct Row3 {
  uint32_t l, c, h;
};

}  // namespace mbk
