// Gaze overlay: the heat map of a gaze track blended onto the source frames, with a disc at the gaze point -- what the reference's
// slowfast/visualization/visualization.py (vis_inference, vis_video_forecasting) draws with cv2: heat map resized to the frame,
// JET colours, 0.6 frame + 0.4 heat, a filled green circle.  Here the map (S/4 x S/4 cells, the `rescaled` of gaze_decode /
// gaze_track) lives on the S x S crop the model saw, so the kernel inverts the test-mode resize and crop per pixel: the params row
// of the sampler says where on the source frame the crop lies.  include/csts_hip.h states the rule.
//
// A pure streaming kernel: 3 bytes in and 3 bytes out per pixel, everything else comes from LDS.  A workgroup owns OV_ROWS rows
// of one frame.  It stages the frame's map, a 256-entry table alpha * JET(q), one entry per row of its band (inside-y, map rows,
// vertical weight) and one per column (inside-x, map columns, horizontal weight) -- the 64-bit coordinate arithmetic runs once
// per row and column, never per pixel.  Then a wave walks one row at a time: on the vector path a lane owns 4 pixels = 12 bytes =
// one 96-bit load and one 96-bit store (W % 4 == 0 keeps every row dword-aligned), on the byte path one pixel.  Both paths call
// the same ov_shade(), so their bytes agree.  Rows that neither touch the crop nor the marker are copied (or skipped in place).
#include "common.h"

namespace {

constexpr int OV_ROWS = 32;                      // frame rows per workgroup, 8 per wave
constexpr int OV_MAX_W = 8192;                   // one 8-byte column entry each in LDS
constexpr uint32_t OV_OUTSIDE = 0xffffffffu;     // column / row entry of a pixel outside the crop

typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));

struct OvAxis { int i0, i1; float lam; bool inside; };

// One axis of the rule, exactly: source pixel p of an extent E that the sampler resized to ne and cropped at [o, o + S), on a map
// axis of m cells.  The position (((p + 0.5) ne / E - 0.5 - o) + 0.5) m / S - 0.5 is the rational A / D below.
__device__ inline OvAxis ov_axis(int p, int E, int ne, int o, int S, int m) {
  const int64_t c = (int64_t)(2 * p + 1) * ne, E2 = 2 * (int64_t)E;
  OvAxis a;
  a.inside = c >= o * E2 && c < (int64_t)(o + S) * E2;
  const int64_t D = E2 * S, A = (c - o * E2) * m - (int64_t)E * S;
  a.i0 = 0;
  a.lam = 0.f;
  if (A > 0) {                                   // src = max(A / D, 0)
    const int64_t q = A / D;
    a.i0 = (int)(q < m - 1 ? q : m - 1);
    a.lam = (float)(A - q * D) / (float)D;
  }
  a.i1 = min(a.i0 + 1, m - 1);
  return a;
}

struct OvRow { uint32_t o0, o1; float ly; int pad_; };      // o0 == OV_OUTSIDE: the row misses the crop; else LDS offsets of the map rows

// one pixel inside the crop: rgb = r | g << 8 | b << 16
__device__ __forceinline__ uint32_t ov_shade(uint32_t rgb, const OvRow& r, uint2 col, const float* map, const float* lut, float oma) {
  const uint32_t j0 = col.x & 0xffffu, j1 = col.x >> 16;
  const float lx = __uint_as_float(col.y);
  const float m00 = map[r.o0 + j0], m01 = map[r.o0 + j1], m10 = map[r.o1 + j0], m11 = map[r.o1 + j1];
  const float top = fmaf(lx, m01 - m00, m00), bot = fmaf(lx, m11 - m10, m10);
  const float v = fmaf(r.ly, bot - top, top);
  const int q = min(255, (int)(v * 255.0f));
  const float* h = lut + 3 * max(q, 0);
  const uint32_t cr = (uint32_t)rintf(oma * (float)(rgb & 0xffu) + h[0]);
  const uint32_t cg = (uint32_t)rintf(oma * (float)((rgb >> 8) & 0xffu) + h[1]);
  const uint32_t cb = (uint32_t)rintf(oma * (float)((rgb >> 16) & 0xffu) + h[2]);
  return cr | (cg << 8) | (cb << 16);
}

// grid N * ceil(H / OV_ROWS), 256 threads; dynamic LDS: OV_ROWS row entries, the JET table, the map, W column entries
template <bool VEC>
__global__ __launch_bounds__(256) void gaze_overlay_kernel(const uint8_t* frames, const float* __restrict__ rescaled,
                                                           const int* __restrict__ centers, const int* __restrict__ params,
                                                           uint8_t* out, int bands, int H, int W, int S, int mh, int mw, float alpha,
                                                           int radius) {
  extern __shared__ __align__(16) uint8_t lds[];
  OvRow* rows = reinterpret_cast<OvRow*>(lds);
  float* lut = reinterpret_cast<float*>(rows + OV_ROWS);
  float* map = lut + 256 * 3;                                   // 16-byte aligned
  uint2* cols = reinterpret_cast<uint2*>(map + ((mh * mw + 1) & ~1));
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t n = blockIdx.x / bands;
  const int Y0 = (blockIdx.x % bands) * OV_ROWS;
  const int nrows = min(OV_ROWS, H - Y0);
  const int64_t band_off = (n * H + Y0) * W * 3;
  const uint8_t* src = frames + band_off;
  uint8_t* dst = out + band_off;
  const bool in_place = src == dst;
  const int64_t row_bytes = (int64_t)W * 3;

  const int cX = centers ? centers[2 * n] : 0, cY = centers ? centers[2 * n + 1] : 0;
  const bool marked = centers && cX >= 0;
  const int nh = params[0], nw = params[1], y0 = params[2], x0 = params[3];
  const bool crop = (!centers || cX >= 0) && nh >= S && nw >= S && nh <= (1 << 24) && nw <= (1 << 24) && y0 >= 0 && x0 >= 0 &&
                    y0 <= nh - S && x0 <= nw - S;

  if (crop) {                                                   // uniform over the workgroup
    const int cells = mh * mw;
    const float* m = rescaled + n * cells;
    if ((cells & 3) == 0 && (reinterpret_cast<uintptr_t>(m) & 15) == 0) {
      for (int k = tid * 4; k < cells; k += 256 * 4) *reinterpret_cast<float4*>(map + k) = *reinterpret_cast<const float4*>(m + k);
    } else {
      for (int k = tid; k < cells; k += 256) map[k] = m[k];
    }
    {                                                           // alpha * JET(q), q = tid
      const int q4 = 4 * tid;
      lut[3 * tid] = alpha * (float)min(max(383 - abs(q4 - 765), 0), 255);
      lut[3 * tid + 1] = alpha * (float)min(max(383 - abs(q4 - 510), 0), 255);
      lut[3 * tid + 2] = alpha * (float)min(max(383 - abs(q4 - 255), 0), 255);
    }
    for (int X = tid; X < W; X += 256) {
      const OvAxis a = ov_axis(X, W, nw, x0, S, mw);
      cols[X] = a.inside ? make_uint2((uint32_t)a.i0 | ((uint32_t)a.i1 << 16), __float_as_uint(a.lam)) : make_uint2(OV_OUTSIDE, 0u);
    }
  }
  if (tid < nrows) {
    OvRow r = {OV_OUTSIDE, 0u, 0.f, 0};
    if (crop) {
      const OvAxis a = ov_axis(Y0 + tid, H, nh, y0, S, mh);
      if (a.inside) r = {(uint32_t)(a.i0 * mw), (uint32_t)(a.i1 * mw), a.lam, 0};
    }
    rows[tid] = r;
  }
  __syncthreads();

  const float oma = 1.0f - alpha;
  const int64_t r2 = (int64_t)radius * radius;
  for (int ry = wv; ry < nrows; ry += 4) {                      // everything about the row is wave-uniform
    const OvRow r = rows[ry];
    const bool heat = r.o0 != OV_OUTSIDE;
    const int64_t dy = (int64_t)(Y0 + ry) - cY;
    const bool disc = marked && dy >= -(int64_t)radius && dy <= (int64_t)radius;
    const int64_t dx_max2 = r2 - dy * dy;                       // the disc covers (X - cX)^2 <= dx_max2 on this row
    if (!heat && !disc && in_place) continue;
    const uint8_t* s = src + ry * row_bytes;
    uint8_t* d = dst + ry * row_bytes;
    if (VEC) {
      for (int g = lane; g < (W >> 2); g += 64) {
        u32x3 v = *reinterpret_cast<const u32x3_a4*>(s + 12 * g);
        if (heat || disc) {
          uint32_t p[4] = {v.x & 0xffffffu, (v.x >> 24) | ((v.y & 0xffffu) << 8), (v.y >> 16) | ((v.z & 0xffu) << 16), v.z >> 8};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int X = 4 * g + k;
            if (heat) {
              const uint2 col = cols[X];
              if (col.x != OV_OUTSIDE) p[k] = ov_shade(p[k], r, col, map, lut, oma);
            }
            if (disc) {
              const int64_t dx = (int64_t)X - cX;
              if (dx >= -(int64_t)radius && dx <= (int64_t)radius && dx * dx <= dx_max2) p[k] = 0x00ff00u;
            }
          }
          v.x = p[0] | (p[1] << 24);
          v.y = (p[1] >> 8) | (p[2] << 16);
          v.z = (p[2] >> 16) | (p[3] << 8);
        }
        *reinterpret_cast<u32x3_a4*>(d + 12 * g) = v;
      }
    } else {
      for (int X = lane; X < W; X += 64) {
        uint32_t p = (uint32_t)s[3 * X] | ((uint32_t)s[3 * X + 1] << 8) | ((uint32_t)s[3 * X + 2] << 16);
        if (heat) {
          const uint2 col = cols[X];
          if (col.x != OV_OUTSIDE) p = ov_shade(p, r, col, map, lut, oma);
        }
        if (disc) {
          const int64_t dx = (int64_t)X - cX;
          if (dx >= -(int64_t)radius && dx <= (int64_t)radius && dx * dx <= dx_max2) p = 0x00ff00u;
        }
        d[3 * X] = (uint8_t)p;
        d[3 * X + 1] = (uint8_t)(p >> 8);
        d[3 * X + 2] = (uint8_t)(p >> 16);
      }
    }
  }
}

}  // namespace

extern "C" int csts_gaze_overlay(const uint8_t* frames_nhwc, const float* rescaled, const int* centers, const int* params,
                                 uint8_t* out, int64_t N, int H, int W, int S, int mh, int mw, float alpha, int radius,
                                 hipStream_t stream) {
  CSTS_REQUIRE(frames_nhwc && rescaled && params && out, "bad args (frames, rescaled, params and out must not be NULL)");
  CSTS_REQUIRE(N >= 1 && H >= 1 && H <= 65535 && W >= 1 && W <= OV_MAX_W && S >= 1 && S <= 4096,
               "bad sizes (N >= 1, H <= 65535, W <= 8192, S <= 4096)");
  CSTS_REQUIRE(mh >= 1 && mw >= 1 && (int64_t)mh * mw <= CSTS_GAZE_DECODE_MAX_HW, "1 <= mh * mw <= CSTS_GAZE_DECODE_MAX_HW (the map is staged in LDS)");
  CSTS_REQUIRE(alpha >= 0.f && alpha <= 1.f, "0 <= alpha <= 1");
  CSTS_REQUIRE(radius >= 0, "radius >= 0");
  const int64_t bands = cdiv(H, OV_ROWS);
  CSTS_REQUIRE(N * bands < ((int64_t)1 << 31), "N * ceil(H / 32) must stay below 2^31");
  const int lds = OV_ROWS * (int)sizeof(OvRow) + 256 * 3 * (int)sizeof(float) + ((mh * mw + 1) & ~1) * (int)sizeof(float) + W * (int)sizeof(uint2);
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(frames_nhwc) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  const void* fn = vec ? reinterpret_cast<const void*>(&gaze_overlay_kernel<true>) : reinterpret_cast<const void*>(&gaze_overlay_kernel<false>);
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(fn, lds), "LDS opt-in");
  if (vec) hipLaunchKernelGGL(gaze_overlay_kernel<true>, dim3((unsigned)(N * bands)), dim3(256), lds, stream, frames_nhwc, rescaled,
                              centers, params, out, (int)bands, H, W, S, mh, mw, alpha, radius);
  else hipLaunchKernelGGL(gaze_overlay_kernel<false>, dim3((unsigned)(N * bands)), dim3(256), lds, stream, frames_nhwc, rescaled,
                          centers, params, out, (int)bands, H, W, S, mh, mw, alpha, radius);
  CSTS_LAUNCH_CHECK();
  return 0;
}
