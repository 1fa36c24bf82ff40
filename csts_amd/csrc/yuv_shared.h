// 4:2:0 YUV pictures (NV12, I420): the colour rule of include/csts_hip.h as one __host__ __device__ pixel function, the byte
// staging the kernels of yuv.hip share, and sample_rows_yuv, the 4:2:0 twin of sample_rows (spatial_shared.h).
#pragma once
#include "spatial_shared.h"

namespace {

// {CY, CRV, CGU, CGV, CBU} = round(c * 2^20) and the luma offset of one (matrix, range)
struct YuvCoef {
  int cy, crv, cgu, cgv, cbu, yoff;
};

inline bool yuv_args_ok(int layout, int matrix) {
  return (layout == CSTS_YUV_NV12 || layout == CSTS_YUV_I420) && (matrix == CSTS_YUV_BT601 || matrix == CSTS_YUV_BT709);
}

inline YuvCoef yuv_coef(int matrix, int full_range) {
  if (matrix == CSTS_YUV_BT709)
    return full_range ? YuvCoef{1048576, 1651297, -196424, -490864, 1945738, 0}
                      : YuvCoef{1220945, 1879825, -223607, -558796, 2215014, 16};
  return full_range ? YuvCoef{1048576, 1470104, -360853, -748826, 1858077, 0}
                    : YuvCoef{1220945, 1673555, -410793, -852458, 2115221, 16};
}

__host__ __device__ __forceinline__ int yuv_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the rule: three bytes -> R, G, B in [0, 255]; int32 throughout (|accumulator| < 5.74e8), >> arithmetic
__host__ __device__ __forceinline__ void yuv_pixel(const YuvCoef& k, int Y, int U, int V, int& R, int& G, int& B) {
  const int y = k.cy * (Y - k.yoff) + (1 << 19), u = U - 128, v = V - 128;
  R = yuv_clamp8((y + k.crv * v) >> 20);
  G = yuv_clamp8((y + k.cgu * u + k.cgv * v) >> 20);
  B = yuv_clamp8((y + k.cbu * u) >> 20);
}

// rgb_to_yuv, the inverse rule of include/csts_hip.h: {yr, yg, yb | ur, ug, ub | vr, vg, vb} = round(c * 2^20) of the real-valued
// matrix of one (matrix, range) and the luma offset
struct RgbCoef {
  int yr, yg, yb, ur, ug, ub, vr, vg, vb, yoff;
};

inline RgbCoef rgb_coef(int matrix, int full_range) {
  if (matrix == CSTS_YUV_BT709)
    return full_range ? RgbCoef{222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074, 0}
                      : RgbCoef{191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230, 16};
  return full_range ? RgbCoef{313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262, 0}
                    : RgbCoef{269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897, 16};
}

// luma of one pixel, R, G, B in [0, 255]; int32 throughout, >> arithmetic
__host__ __device__ __forceinline__ int rgb_luma(const RgbCoef& k, int R, int G, int B) {
  return yuv_clamp8(((k.yr * R + k.yg * G + k.yb * B + (1 << 19)) >> 20) + k.yoff);
}

// chroma of one 2 x 2 block from the sums of its four pixels, SR, SG, SB in [0, 1020] (|accumulator| <= 2^29 = 524288 * 1020 + 2^21)
__host__ __device__ __forceinline__ void rgb_chroma(const RgbCoef& k, int SR, int SG, int SB, int& U, int& V) {
  U = yuv_clamp8(((k.ur * SR + k.ug * SG + k.ub * SB + (1 << 21)) >> 22) + 128);
  V = yuv_clamp8(((k.vr * SR + k.vg * SG + k.vb * SB + (1 << 21)) >> 22) + 128);
}

// bytes of one frame; H, W even
__host__ __device__ __forceinline__ int64_t yuv_frame_bytes(int64_t H, int64_t W) { return H * W / 2 * 3; }

// Where the H x W picture lies in the tensor that holds it ("decoder surfaces", include/csts_hip.h): the tensor is a tight 4:2:0
// picture of Hs x Ws (pitch Ws, chroma from byte Hs * Ws of a frame), the picture its window at row `top`, column `left`; all even.
// Addresses (frame stride, row and plane offsets) come from here; clamps, scales and LDS sizes from H and W.  A tight picture is
// {H, W, 0, 0}, and then every offset below is the tight one.
struct YuvSurf {
  int Hs, Ws, top, left;
};

__host__ __device__ __forceinline__ YuvSurf yuv_tight(int H, int W) { return YuvSurf{H, W, 0, 0}; }

__host__ __device__ __forceinline__ int64_t yuv_frame_bytes(const YuvSurf& s) { return yuv_frame_bytes(s.Hs, s.Ws); }

// byte of luma (y, 0) of the picture, counted from the frame's first byte
__host__ __device__ __forceinline__ int64_t yuv_luma_row(const YuvSurf& s, int y) { return (int64_t)(s.top + y) * s.Ws + s.left; }

// byte of chroma row cy, pair 0: the U byte; nv12: V follows it, i420: V lies yuv_vplane further on
__host__ __device__ __forceinline__ int64_t yuv_chroma_row(const YuvSurf& s, int cy, bool nv12) {
  const int64_t r = (s.top >> 1) + cy, c0 = (int64_t)s.Hs * s.Ws;
  return nv12 ? c0 + r * s.Ws + s.left : c0 + r * (s.Ws >> 1) + (s.left >> 1);
}

__host__ __device__ __forceinline__ int64_t yuv_vplane(const YuvSurf& s) { return (int64_t)(s.Hs >> 1) * (s.Ws >> 1); }

// the window of a surface as include/csts_hip.h defines it
inline bool yuv_surf_ok(int H, int W, const YuvSurf& s) {
  return ((s.Hs | s.Ws | s.top | s.left | H | W) & 1) == 0 && H >= 2 && W >= 2 && s.top >= 0 && s.left >= 0 && s.Hs >= H &&
         s.Ws >= W && s.Ws <= CSTS_YUV_MAX_WS && s.top <= s.Hs - H && s.left <= s.Ws - W;
}
#define YUV_SURF_MSG "bad window (top, left, H, W even, H, W >= 2, inside the Hs x Ws surface; Ws <= CSTS_YUV_MAX_WS = 32768)"

// Stage the bytes [beg, end) of src into dst as the 16-byte chunks of src that cover them (src is 16-byte aligned, offsets count
// from it; dst is 16-byte aligned LDS of at least end - beg + 30 bytes rounded up to 16); returns where byte `beg` lies in dst.
// Only bytes inside [lo, hi) are read (zeros stand in for the others).  Called by `nthr` threads numbered `tid`.
__device__ __forceinline__ int yuv_stage(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t beg, int64_t end,
                                         int64_t lo, int64_t hi, int tid, int nthr) {
  const int64_t a0 = beg & ~(int64_t)15, nbytes = ((end + 15) & ~(int64_t)15) - a0;
  for (int64_t k = (int64_t)tid * 16; k < nbytes; k += (int64_t)nthr * 16) {
    const int64_t g = a0 + k;
    if (g >= lo && g + 16 <= hi) {
      *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + g);
    } else {
      for (int q = 0; q < 16; ++q) dst[k + q] = (g + q >= lo && g + q < hi) ? src[g + q] : 0;
    }
  }
  return (int)(beg - a0);
}

// The way back: the bytes [beg, end) of img, an LDS image laid out from a 16-byte aligned global address g (byte c of img belongs
// at g + c), written as 16-byte chunks; the ragged first and last chunk go byte by byte, so no byte outside [beg, end) is written
// (a neighbouring workgroup owns those).  Called by `nthr` threads numbered `tid`.
__device__ __forceinline__ void yuv_unstage(uint8_t* g, const uint8_t* img, int beg, int end, int tid, int nthr) {
  for (int c = tid * 16; c < end; c += nthr * 16) {
    if (c >= beg && c + 16 <= end) {
      *reinterpret_cast<uint4*>(g + c) = *reinterpret_cast<const uint4*>(img + c);
    } else {
      for (int q = 0; q < 16; ++q)
        if (c + q >= beg && c + q < end) g[c + q] = img[c + q];
    }
  }
}

// dynamic LDS of a 4:2:0 sample launch for source rows of up to W pixels.  Per wave: two luma rows of lcap bytes, then the chroma of
// both rows: two interleaved rows of lcap bytes (nv12) or U, U, V, V rows of ccap bytes (i420); 2 lcap <= 4 ccap.  About
// 4 W + 200 bytes against the RGB pass's 2 (3 W + 30).
__host__ __device__ inline int sample_yuv_lds_bytes(int W, int* lcap, int* ccap) {
  *lcap = (W + 30 + 15) / 16 * 16;
  *ccap = (W / 2 + 30 + 15) / 16 * 16;
  return SAMPLE_ROWS * (2 * *lcap + 4 * *ccap);
}

// sample_rows for a recording of 4:2:0 frames (the H x W pictures of the surfaces sf; H, W even -- the caller passes bad otherwise,
// and a window that lies inside its surface): the same geometry, the same staging and, after the four taps of a pixel are converted
// to integer R, G, B, the same fp32 expressions in the same order, so the output equals sample_rows on the converted recording bit
// for bit.  lds: sample_yuv_lds_bytes.
__device__ __forceinline__ void sample_rows_yuv(const uint8_t* __restrict__ src, int64_t src_bytes, int64_t base, int64_t frame,
                                                int H, int W, const YuvSurf& sf, const int* __restrict__ par, bool bad, float* __restrict__ out, int b,
                                                int t, int T, int S, int lcap, int ccap, int layout, const YuvCoef& k, float3 mean,
                                                float3 inv_std, uint8_t* lds) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * SAMPLE_ROWS + wv;                 // output row of this wave
  const int nh = par[0], nw = par[1], y0 = par[2], x0 = par[3], flip = par[4];
  const int64_t plane = (int64_t)S * S;
  float* o0 = out + ((int64_t)b * 3 * T + t) * plane + (int64_t)i * S;      // channel c at o0 + c * T * plane
  const int64_t cstride = (int64_t)T * plane;
  const bool row_ok = i < S;
  if (bad || nh < S || nw < S || y0 < 0 || x0 < 0 || y0 > nh - S || x0 > nw - S) {
    if (row_ok)
      for (int j = lane; j < S; j += 64)
        for (int c = 0; c < 3; ++c) o0[c * cstride + j] = __builtin_nanf("");
    return;                                                    // uniform over the workgroup (one clip)
  }
  const float sy = (float)H / (float)nh, sx = (float)W / (float)nw;   // area_pixel_compute_scale, fp32
  float fy = fmaxf(((float)(y0 + (row_ok ? i : 0)) + 0.5f) * sy - 0.5f, 0.f);
  const int ya = min((int)fy, H - 1), yb = min(ya + 1, H - 1);
  const float ly = fy - (float)ya;
  const int xlo = min((int)fmaxf(((float)x0 + 0.5f) * sx - 0.5f, 0.f), W - 1);
  const int xhi = min((int)fmaxf(((float)(x0 + S - 1) + 0.5f) * sx - 0.5f, 0.f) + 1, W - 1);
  const int clo = xlo >> 1, chi = xhi >> 1;                    // chroma columns the span reads
  uint8_t* rows = lds + wv * (2 * lcap + 4 * ccap);
  const bool nv12 = layout == CSTS_YUV_NV12;
  // LDS byte of luma x of row r: yo[r] + x; of the chroma pair cx: nv12 uo[r] + 2 cx (U), + 1 (V); i420 uo[r] + cx, vo[r] + cx
  int yo[2], uo[2], vo[2];
  const int64_t f0 = base + frame * yuv_frame_bytes(sf);
  for (int r = 0; r < 2; ++r) {
    const int y = r ? yb : ya;
    const int64_t l0 = f0 + yuv_luma_row(sf, y), q0 = f0 + yuv_chroma_row(sf, y >> 1, nv12);
    if (row_ok) yo[r] = r * lcap + yuv_stage(rows + r * lcap, src, l0 + xlo, l0 + xhi + 1, 0, src_bytes, lane, 64) - xlo;
    if (nv12) {
      uint8_t* d = rows + 2 * lcap + r * lcap;
      if (row_ok) uo[r] = (int)(d - rows) + yuv_stage(d, src, q0 + 2 * clo, q0 + 2 * chi + 2, 0, src_bytes, lane, 64) - 2 * clo;
    } else {
      const int64_t q1 = q0 + yuv_vplane(sf);
      uint8_t* du = rows + 2 * lcap + r * ccap;
      uint8_t* dv = du + 2 * ccap;
      if (row_ok) {
        uo[r] = (int)(du - rows) + yuv_stage(du, src, q0 + clo, q0 + chi + 1, 0, src_bytes, lane, 64) - clo;
        vo[r] = (int)(dv - rows) + yuv_stage(dv, src, q1 + clo, q1 + chi + 1, 0, src_bytes, lane, 64) - clo;
      }
    }
  }
  __syncthreads();
  if (!row_ok) return;
  const float h1 = ly, h0 = 1.f - ly;
  const float m[3] = {mean.x, mean.y, mean.z}, is[3] = {inv_std.x, inv_std.y, inv_std.z};
  for (int j0 = lane * 4; j0 < S; j0 += 64 * 4) {
    float v[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = min(j0 + q, S - 1);
      const int X = x0 + (flip ? S - 1 - j : j);
      const float fx = fmaxf(((float)X + 0.5f) * sx - 0.5f, 0.f);
      const int xa = min((int)fx, W - 1), xb = min(xa + 1, W - 1);
      const float w1 = fx - (float)xa, w0 = 1.f - w1;
      float tap[2][2][3];                                      // [row][xa | xb][channel], integers in fp32
#pragma unroll
      for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int x = e ? xb : xa, cx = x >> 1;
          const int Y = rows[yo[r] + x];
          const int U = nv12 ? rows[uo[r] + 2 * cx] : rows[uo[r] + cx];
          const int V = nv12 ? rows[uo[r] + 2 * cx + 1] : rows[vo[r] + cx];
          int R, G, B;
          yuv_pixel(k, Y, U, V, R, G, B);
          tap[r][e][0] = (float)R;
          tap[r][e][1] = (float)G;
          tap[r][e][2] = (float)B;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p = tap[0][0][c] * w0 + tap[0][1][c] * w1;
        const float n = tap[1][0][c] * w0 + tap[1][1][c] * w1;
        v[c][q] = ((p * h0 + n * h1) / 255.0f - m[c]) * is[c];
      }
    }
    if ((S & 3) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(o0 + c * cstride + j0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
      for (int q = 0; q < 4 && j0 + q < S; ++q)
        for (int c = 0; c < 3; ++c) o0[c * cstride + j0 + q] = v[c][q];
    }
  }
}

}  // namespace
