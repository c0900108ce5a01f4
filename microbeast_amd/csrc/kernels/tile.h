// Device-side building blocks of the conv tile kernels (conv.hip, trunk.hip, resblock.hip and
// the other MFMA kernels): the operand fragment, the pixel-index split, the halo'd-tile window
// offset, the dgrad / forward MFMA block, the weight-gradient K block and the relu-gate /
// residual epilogue steps. Every helper is a forced inline of the code its callers used to
// write out, so the emitted instructions are the callers' own.
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

}  // namespace mbk
