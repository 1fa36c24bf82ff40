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
// gaze_overlay_yuv_kernel (below) draws the same picture onto 4:2:0 frames and writes 4:2:0 frames, through the same ov_axis and
// ov_shade.
// group_gaze_overlay_kernel / group_gaze_overlay_yuv_kernel draw the frames of several jobs, each of its own H x W, in one launch
// from a job table, and group_points_source_kernel computes their marker centres: what a live group needs per tick.
#include <algorithm>
#include <vector>

#include "yuv_shared.h"

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

// One band of one frame, by the 256 threads of a workgroup: rows [Y0, Y0 + nrows) of a frame of H x W, src / dst the first byte of
// the band in the frame and in the output, m the frame's map, (cX, cY) its marker centre (marked: it has one), crop: the frame is
// drawn and (nh, nw, y0, x0) hold an S x S crop.  Everything but the pixels is uniform over the workgroup.  Dynamic LDS: OV_ROWS
// row entries, the JET table, the map, W column entries.  gaze_overlay_kernel and group_gaze_overlay_kernel are this function
// under two ways of finding the band, so their bytes agree.
template <bool VEC>
__device__ __forceinline__ void ov_band(uint8_t* lds, const uint8_t* src, uint8_t* dst, const float* __restrict__ m, int cX, int cY,
                                        bool marked, bool crop, int nh, int nw, int y0, int x0, int Y0, int nrows, int H, int W, int S,
                                        int mh, int mw, float alpha, int radius) {
  OvRow* rows = reinterpret_cast<OvRow*>(lds);
  float* lut = reinterpret_cast<float*>(rows + OV_ROWS);
  float* map = lut + 256 * 3;                                   // 16-byte aligned
  uint2* cols = reinterpret_cast<uint2*>(map + ((mh * mw + 1) & ~1));
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool in_place = src == dst;
  const int64_t row_bytes = (int64_t)W * 3;

  if (crop) {                                                   // uniform over the workgroup
    const int cells = mh * mw;
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

// whether a frame with these centre and params is drawn inside its crop (the rule of include/csts_hip.h)
__device__ __forceinline__ bool ov_crop(bool centers, int cX, int nh, int nw, int y0, int x0, int S) {
  return (!centers || cX >= 0) && nh >= S && nw >= S && nh <= (1 << 24) && nw <= (1 << 24) && y0 >= 0 && x0 >= 0 && y0 <= nh - S &&
         x0 <= nw - S;
}

// grid N * ceil(H / OV_ROWS), 256 threads; dynamic LDS as ov_band states it
template <bool VEC>
__global__ __launch_bounds__(256) void gaze_overlay_kernel(const uint8_t* frames, const float* __restrict__ rescaled,
                                                           const int* __restrict__ centers, const int* __restrict__ params,
                                                           uint8_t* out, int bands, int H, int W, int S, int mh, int mw, float alpha,
                                                           int radius) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int64_t n = blockIdx.x / bands;
  const int Y0 = (blockIdx.x % bands) * OV_ROWS;
  const int64_t band_off = (n * H + Y0) * W * 3;
  const int cX = centers ? centers[2 * n] : 0, cY = centers ? centers[2 * n + 1] : 0;
  const int nh = params[0], nw = params[1], y0 = params[2], x0 = params[3];
  ov_band<VEC>(lds, frames + band_off, out + band_off, rescaled + n * mh * mw, cX, cY, centers && cX >= 0,
               ov_crop(centers != nullptr, cX, nh, nw, y0, x0, S), nh, nw, y0, x0, Y0, min(OV_ROWS, H - Y0), H, W, S, mh, mw, alpha,
               radius);
}

// ---- the same picture drawn in 4:2:0 (NV12 / I420 in, the same layout out; include/csts_hip.h states the rule) ----------------------
// 1.5 bytes in and 1.5 bytes out per pixel; the RGB picture exists only in registers.  A workgroup owns OVY_BAND pairs of luma rows
// of one frame and the chroma rows those pairs share (nv12: chroma row cy belongs to row pair cy; i420: row cy of U and row cy of
// V), so no workgroup reads a byte another one writes and in place is legal.  It stages map, alpha * JET, row and column entries as
// gaze_overlay_kernel does (ovy_tables).  The unit of work is one 2 x 2 block (ovy_block): yuv_pixel on its four pixels, ov_shade /
// the disc on the drawn ones, rgb_luma on the drawn ones, rgb_chroma on the sums if any is drawn.  Two kernels feed it:
//   gaze_overlay_yuv_vec_kernel   W % 4 == 0, frames and out 4-byte aligned (what a decoder delivers): every luma row, every nv12
//       chroma row starts on a dword and every i420 chroma row on a 2-byte word, so, like the vector path of gaze_overlay_kernel,
//       a wave walks one row pair and a lane owns 4 pixels of both rows and their two chroma pairs: three 4-byte loads, two blocks,
//       three 4-byte stores (i420: 2 + 2 bytes of chroma), no LDS traffic for the pixels and no barrier after the tables;
//   gaze_overlay_yuv_kernel       any byte alignment (a recording inside a larger buffer, W = 2 mod 4): OVY_PAIRS row pairs of a
//       tile at a time, the source bytes staged in LDS (yuv_stage: 16-byte chunks from any byte), a thread per block, the output
//       bytes built in LDS images laid out from the output addresses and written back as 16-byte chunks (yuv_unstage; the ragged
//       first and last chunk byte by byte, only bytes the workgroup owns).  All reads of a pass come before its barrier, all its
//       writes after.
// Both give the same bytes.  Row pairs that touch neither crop nor disc are copied, or skipped in place.
// (Measured on 16 nv12 frames of 1088 x 1080: the staged kernel alone took 150 us against 114 us of yuv_to_rgb + gaze_overlay,
// bound by its barrier phases at two workgroups a CU, not by bytes; hence the vector kernel.  tools/overlay_yuv_bench.py.)
constexpr int OVY_BAND = 16;                     // row pairs per workgroup: OV_ROWS luma rows
constexpr int OVY_PAIRS = 2;                     // row pairs per pass of the staged kernel
constexpr int OVY_TW = 2048;                     // pixels of the widest tile of the staged kernel

// what a workgroup knows about its frame: marker, crop (as gaze_overlay_kernel derives them from centers and params)
struct OvyFrame {
  int cX, cY, nh, nw, y0, x0;
  bool marked, crop;
};

// n: the frame's row of centers; (nh, nw, y0, x0): its params
__device__ __forceinline__ OvyFrame ovy_frame(const int* __restrict__ centers, int64_t n, int nh, int nw, int y0, int x0, int S) {
  OvyFrame f;
  f.cX = centers ? centers[2 * n] : 0;
  f.cY = centers ? centers[2 * n + 1] : 0;
  f.marked = centers && f.cX >= 0;
  f.nh = nh, f.nw = nw, f.y0 = y0, f.x0 = x0;
  f.crop = ov_crop(centers != nullptr, f.cX, nh, nw, y0, x0, S);
  return f;
}

__device__ __forceinline__ OvyFrame ovy_frame(const int* __restrict__ centers, const int* __restrict__ params, int64_t n, int S) {
  return ovy_frame(centers, n, params[0], params[1], params[2], params[3], S);
}

// The tables of a workgroup, staged by its 256 threads (no barrier inside): the frame's map m, alpha * JET(q), one entry per luma
// row [Y0, Y0 + nrows) and one per column [X0, X0 + tw).  map, lut and cols are written only when the frame has a crop.
__device__ __forceinline__ void ovy_tables(OvRow* rows, float* lut, float* map, uint2* cols, const float* __restrict__ m,
                                           const OvyFrame& f, float alpha, int Y0, int nrows, int X0, int tw, int H, int W, int S,
                                           int mh, int mw, int tid) {
  if (f.crop) {                                                 // uniform over the workgroup
    const int cells = mh * mw;
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
    for (int j = tid; j < tw; j += 256) {
      const OvAxis a = ov_axis(X0 + j, W, f.nw, f.x0, S, mw);
      cols[j] = a.inside ? make_uint2((uint32_t)a.i0 | ((uint32_t)a.i1 << 16), __float_as_uint(a.lam)) : make_uint2(OV_OUTSIDE, 0u);
    }
  }
  if (tid < nrows) {
    OvRow r = {OV_OUTSIDE, 0u, 0.f, 0};
    if (f.crop) {
      const OvAxis a = ov_axis(Y0 + tid, H, f.nh, f.y0, S, mh);
      if (a.inside) r = {(uint32_t)(a.i0 * mw), (uint32_t)(a.i1 * mw), a.lam, 0};
    }
    rows[tid] = r;
  }
}

// one pair of luma rows: uniform over whoever walks it
struct OvyPair {
  OvRow rw[2];
  bool heat[2], disc[2], drawn;
  int64_t dxm[2];                                               // the disc covers (X - cX)^2 <= dxm on that row
};

// rows: the entries of luma rows 2 cy and 2 cy + 1
__device__ __forceinline__ OvyPair ovy_pair(const OvRow* rows, int cy, const OvyFrame& f, int radius) {
  OvyPair p;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    p.rw[r] = rows[r];
    p.heat[r] = p.rw[r].o0 != OV_OUTSIDE;
    const int64_t dy = (int64_t)(2 * cy + r) - f.cY;
    p.disc[r] = f.marked && dy >= -(int64_t)radius && dy <= (int64_t)radius;
    p.dxm[r] = (int64_t)radius * radius - dy * dy;
  }
  p.drawn = p.heat[0] || p.heat[1] || p.disc[0] || p.disc[1];
  return p;
}

// The 2 x 2 block at columns X, X + 1 (X even) of a drawn pair: Y[r][e], U, V come in as the source bytes and go out as the bytes to
// write.  cols: the column entries, cols[0] that of column X (read only where a row has heat).
__device__ __forceinline__ void ovy_block(int (&Y)[2][2], int& U, int& V, int X, const OvyPair& p, const uint2* cols, int cX,
                                          int radius, const float* map, const float* lut, float oma, const YuvCoef& kf,
                                          const RgbCoef& kr) {
  uint2 col[2] = {make_uint2(OV_OUTSIDE, 0u), make_uint2(OV_OUTSIDE, 0u)};
  if (p.heat[0] || p.heat[1]) {
    col[0] = cols[0];
    col[1] = cols[1];
  }
  bool dot[2][2], m[2][2];
  bool any = false;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int64_t dx = (int64_t)(X + e) - cX;
      dot[r][e] = p.disc[r] && dx >= -(int64_t)radius && dx <= (int64_t)radius && dx * dx <= p.dxm[r];
      m[r][e] = dot[r][e] || (p.heat[r] && col[e].x != OV_OUTSIDE);
      any = any || m[r][e];
    }
  }
  if (!any) return;
  int SR = 0, SG = 0, SB = 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      int R, G, B;
      yuv_pixel(kf, Y[r][e], U, V, R, G, B);
      if (m[r][e]) {
        uint32_t px = (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
        if (p.heat[r] && col[e].x != OV_OUTSIDE) px = ov_shade(px, p.rw[r], col[e], map, lut, oma);
        if (dot[r][e]) px = 0x00ff00u;
        R = (int)(px & 0xffu);
        G = (int)((px >> 8) & 0xffu);
        B = (int)((px >> 16) & 0xffu);
        Y[r][e] = rgb_luma(kr, R, G, B);
      }
      SR += R;
      SG += G;
      SB += B;
    }
  }
  rgb_chroma(kr, SR, SG, SB, U, V);
}

// The row pairs [P0, P0 + OVY_BAND) of one frame on the vector path, by the 256 threads of a workgroup: frames / out the first byte of
// the FRAME (4-byte aligned, W % 4 == 0) and of its output, m its map, f what ovy_frame says of it.  The frame is the H x W window of
// the surface sf (Ws % 4 == 0, left % 4 == 0: every row of the window starts on a dword as well); out is a surface like it.  Dynamic LDS: 2 OVY_BAND row
// entries, the JET table, the map, W column entries.  gaze_overlay_yuv_vec_kernel and group_gaze_overlay_yuv_kernel are this
// function under two ways of finding the frame, so their bytes agree.
template <bool NV12>
__device__ __forceinline__ void ovy_vec_band(uint8_t* lds, const uint8_t* frames, uint8_t* out, const float* __restrict__ m,
                                             const OvyFrame& f, int P0, int H, int W, const YuvSurf& sf, int S, int mh, int mw,
                                             float alpha, int radius, const YuvCoef& kf, const RgbCoef& kr) {
  OvRow* rows = reinterpret_cast<OvRow*>(lds);
  float* lut = reinterpret_cast<float*>(rows + 2 * OVY_BAND);
  float* map = lut + 256 * 3;                                   // 16-byte aligned
  uint2* cols = reinterpret_cast<uint2*>(map + ((mh * mw + 3) & ~3));
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int npairs = min(OVY_BAND, (H >> 1) - P0);
  const int Ws = sf.Ws;
  const bool in_place = frames == out;
  if (!f.crop && !f.marked && in_place) return;                 // uniform: nothing of this frame is drawn
  ovy_tables(rows, lut, map, cols, m, f, alpha, 2 * P0, 2 * npairs, 0, W, H, W, S, mh, mw, tid);
  __syncthreads();

  const float oma = 1.0f - alpha;
  const int64_t vplane = yuv_vplane(sf);
  for (int pr = wv; pr < npairs; pr += 4) {                     // everything about the row pair is wave-uniform
    const int cy = P0 + pr;
    const OvyPair p = ovy_pair(rows + 2 * pr, cy, f, radius);
    if (!p.drawn && in_place) continue;
    const int64_t l0 = yuv_luma_row(sf, 2 * cy), q0 = yuv_chroma_row(sf, cy, NV12);
    for (int g = lane; g < (W >> 2); g += 64) {
      uint32_t a = *reinterpret_cast<const uint32_t*>(frames + l0 + 4 * g);
      uint32_t b = *reinterpret_cast<const uint32_t*>(frames + l0 + Ws + 4 * g);
      uint32_t c;                                               // U0 | V0 << 8 | U1 << 16 | V1 << 24
      if (NV12) {
        c = *reinterpret_cast<const uint32_t*>(frames + q0 + 4 * g);
      } else {
        const uint32_t u = *reinterpret_cast<const uint16_t*>(frames + q0 + 2 * g);
        const uint32_t v = *reinterpret_cast<const uint16_t*>(frames + q0 + vplane + 2 * g);
        c = (u & 0xffu) | ((v & 0xffu) << 8) | ((u >> 8) << 16) | ((v >> 8) << 24);
      }
      if (p.drawn) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int s = 16 * k;
          int Y[2][2] = {{(int)((a >> s) & 0xffu), (int)((a >> (s + 8)) & 0xffu)}, {(int)((b >> s) & 0xffu), (int)((b >> (s + 8)) & 0xffu)}};
          int U = (int)((c >> s) & 0xffu), V = (int)((c >> (s + 8)) & 0xffu);
          ovy_block(Y, U, V, 4 * g + 2 * k, p, cols + 4 * g + 2 * k, f.cX, radius, map, lut, oma, kf, kr);
          const uint32_t keep = ~(0xffffu << s);
          a = (a & keep) | (((uint32_t)Y[0][0] | ((uint32_t)Y[0][1] << 8)) << s);
          b = (b & keep) | (((uint32_t)Y[1][0] | ((uint32_t)Y[1][1] << 8)) << s);
          c = (c & keep) | (((uint32_t)U | ((uint32_t)V << 8)) << s);
        }
      }
      *reinterpret_cast<uint32_t*>(out + l0 + 4 * g) = a;
      *reinterpret_cast<uint32_t*>(out + l0 + Ws + 4 * g) = b;
      if (NV12) {
        *reinterpret_cast<uint32_t*>(out + q0 + 4 * g) = c;
      } else {
        *reinterpret_cast<uint16_t*>(out + q0 + 2 * g) = (uint16_t)((c & 0xffu) | ((c >> 8) & 0xff00u));
        *reinterpret_cast<uint16_t*>(out + q0 + vplane + 2 * g) = (uint16_t)(((c >> 8) & 0xffu) | ((c >> 16) & 0xff00u));
      }
    }
  }
}

// grid N * bands, 256 threads; W, Ws, left % 4 == 0, frames and out 4-byte aligned; dynamic LDS as ovy_vec_band states it
template <bool NV12>
__global__ __launch_bounds__(256) void gaze_overlay_yuv_vec_kernel(const uint8_t* frames, uint8_t* out, const float* __restrict__ rescaled,
                                                                   const int* __restrict__ centers, const int* __restrict__ params,
                                                                   int bands, int H, int W, YuvSurf sf, int S, int mh, int mw,
                                                                   float alpha, int radius, YuvCoef kf, RgbCoef kr) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int64_t n = blockIdx.x / bands, f0 = n * yuv_frame_bytes(sf);
  const OvyFrame f = ovy_frame(centers, params, n, S);
  ovy_vec_band<NV12>(lds, frames + f0, out + f0, rescaled + n * mh * mw, f, (int)(blockIdx.x % bands) * OVY_BAND, H, W, sf, S, mh, mw,
                     alpha, radius, kf, kr);
}

// ---- the overlays of a group: one launch over jobs of different sizes (include/csts_hip.h, "gaze overlay of a group") --------------
// jobs int64 [njobs][OVG_JOB]: one row per job, read through the scalar path -- every index below is uniform over the workgroup.
// A workgroup finds its job by binary search over the first-workgroup column, then its frame and band inside the job, and from
// there on it is ov_band / ovy_vec_band on that frame: the single-tensor kernels' code, hence their bytes.
constexpr int OVG_JOB = 13;
enum { OVG_SRC = 0, OVG_DST, OVG_K, OVG_H, OVG_W, OVG_NH, OVG_NW, OVG_Y0, OVG_X0, OVG_FLIP, OVG_ROW0, OVG_WG0, OVG_VEC };

// the last job j whose column `col` is <= key; the column ascends and starts at 0 <= key
__device__ __forceinline__ int ovg_find(const int64_t* __restrict__ jobs, int njobs, int col, int64_t key) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[(int64_t)mid * OVG_JOB + col] <= key) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// A workgroup's place in the table: its job row, the frame k of the job and the band of the frame; nullptr (the workgroup writes
// nothing) when the device table does not hold what the launch was sized for: a frame past the job's K, a W wider than the LDS
// of the launch (max_w), a size out of range.
__device__ __forceinline__ const int64_t* ovg_place(const int64_t* __restrict__ jobs, int njobs, int max_w, int64_t* k, int* band) {
  const int64_t* job = jobs + (int64_t)ovg_find(jobs, njobs, OVG_WG0, blockIdx.x) * OVG_JOB;
  const int64_t H = job[OVG_H], W = job[OVG_W], local = (int64_t)blockIdx.x - job[OVG_WG0];
  if (H < 1 || H > 65535 || W < 1 || W > max_w || local < 0) return nullptr;
  const int64_t bands = (H + OV_ROWS - 1) / OV_ROWS;
  *k = local / bands;
  *band = (int)(local % bands);
  return *k < job[OVG_K] ? job : nullptr;
}

// grid = the sum of K * ceil(H / OV_ROWS) over the jobs, 256 threads; dynamic LDS: ov_band's at the widest W of the call (max_w)
__global__ __launch_bounds__(256) void group_gaze_overlay_kernel(const int64_t* __restrict__ jobs, int njobs, int max_w,
                                                                 const float* __restrict__ rescaled, const int* __restrict__ centers,
                                                                 int S, int mh, int mw, float alpha, int radius) {
  extern __shared__ __align__(16) uint8_t lds[];
  int64_t k;
  int band;
  const int64_t* job = ovg_place(jobs, njobs, max_w, &k, &band);
  if (!job) return;
  const int H = (int)job[OVG_H], W = (int)job[OVG_W], Y0 = band * OV_ROWS;
  const int nh = (int)job[OVG_NH], nw = (int)job[OVG_NW], y0 = (int)job[OVG_Y0], x0 = (int)job[OVG_X0];
  const int64_t n = job[OVG_ROW0] + k, band_off = (k * H + Y0) * W * 3;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(job[OVG_SRC]) + band_off;
  uint8_t* dst = reinterpret_cast<uint8_t*>(job[OVG_DST]) + band_off;
  const int cX = centers ? centers[2 * n] : 0, cY = centers ? centers[2 * n + 1] : 0;
  const bool marked = centers && cX >= 0, crop = ov_crop(centers != nullptr, cX, nh, nw, y0, x0, S);
  const float* m = rescaled + n * mh * mw;
  const int nrows = min(OV_ROWS, H - Y0);
  if (job[OVG_VEC]) ov_band<true>(lds, src, dst, m, cX, cY, marked, crop, nh, nw, y0, x0, Y0, nrows, H, W, S, mh, mw, alpha, radius);
  else ov_band<false>(lds, src, dst, m, cX, cY, marked, crop, nh, nw, y0, x0, Y0, nrows, H, W, S, mh, mw, alpha, radius);
}

// the same for 4:2:0 jobs, all on the vector path (the entry refuses a job that is not); grid and LDS as above (ovy_vec_band's)
template <bool NV12>
__global__ __launch_bounds__(256) void group_gaze_overlay_yuv_kernel(const int64_t* __restrict__ jobs, int njobs, int max_w,
                                                                     const float* __restrict__ rescaled,
                                                                     const int* __restrict__ centers, int S, int mh, int mw,
                                                                     float alpha, int radius, YuvCoef kf, RgbCoef kr) {
  extern __shared__ __align__(16) uint8_t lds[];
  int64_t k;
  int band;
  const int64_t* job = ovg_place(jobs, njobs, max_w, &k, &band);
  if (!job || !job[OVG_VEC]) return;
  const int H = (int)job[OVG_H], W = (int)job[OVG_W];
  if ((H & 1) || (W & 3)) return;
  const int64_t n = job[OVG_ROW0] + k, f0 = k * yuv_frame_bytes(H, W);
  const OvyFrame f = ovy_frame(centers, n, (int)job[OVG_NH], (int)job[OVG_NW], (int)job[OVG_Y0], (int)job[OVG_X0], S);
  ovy_vec_band<NV12>(lds, reinterpret_cast<const uint8_t*>(job[OVG_SRC]) + f0, reinterpret_cast<uint8_t*>(job[OVG_DST]) + f0,
                     rescaled + n * mh * mw, f, band * OVY_BAND, H, W, yuv_tight(H, W), S, mh, mw, alpha, radius, kf, kr);
}

// points on the crop -> points on the source frame and marker centres, one thread per row: infer.points_to_source followed by
// infer.marker_centers under the row's job (found by binary search over the first-row column).  Plain IEEE double arithmetic, the
// operations torch performs in torch's order (the file is compiled without contraction): multiply, add, divide; multiply, floor.
__global__ __launch_bounds__(256) void group_points_source_kernel(const int64_t* __restrict__ jobs, int njobs,
                                                                  const float* __restrict__ points, double* __restrict__ points_source,
                                                                  int* __restrict__ centers, int64_t P, int S) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int64_t* job = jobs + (int64_t)ovg_find(jobs, njobs, OVG_ROW0, p) * OVG_JOB;
  const double x = (double)points[2 * p], y = (double)points[2 * p + 1], s = (double)S;
  const double xs = (x * s + (double)job[OVG_X0]) / (double)job[OVG_NW];
  const double ys = (y * s + (double)job[OVG_Y0]) / (double)job[OVG_NH];
  points_source[2 * p] = xs;
  points_source[2 * p + 1] = ys;
  const bool bad = xs != xs || ys != ys;
  centers[2 * p] = bad ? -1 : (int)floor(xs * (double)job[OVG_W]);
  centers[2 * p + 1] = bad ? -1 : (int)floor(ys * (double)job[OVG_H]);
}

// The host copy of a job table, checked row by row as the single-tensor entries check their tensor -> the widest W, or -1.  *rows:
// the sum of K; *grid: the sum of K * bands.
int ovg_check(const int64_t* jobs_host, int njobs, bool yuv, bool pointers, int64_t* rows, int64_t* grid) {
  CSTS_REQUIRE(jobs_host && njobs >= 1 && njobs <= 65535, "the host copy of the job table is missing, or 1 <= njobs <= 65535 fails");
  int64_t P = 0, G = 0, max_w = 0;
  for (int j = 0; j < njobs; ++j) {
    const int64_t* job = jobs_host + (int64_t)j * OVG_JOB;
    const int64_t K = job[OVG_K], H = job[OVG_H], W = job[OVG_W];
    CSTS_REQUIRE(K >= 1 && K < ((int64_t)1 << 31) && H >= 1 && H <= 65535 && W >= 1 && W <= OV_MAX_W,
                 "a job has bad sizes (K >= 1, 1 <= H <= 65535, 1 <= W <= 8192)");
    // the overlays index rescaled / centers with it (rows may be left out between jobs), group_points_source searches it
    CSTS_REQUIRE(pointers ? job[OVG_ROW0] >= P : job[OVG_ROW0] == P,
                 "a job's first row lies before the end of the job before it, or (points) is not the number of rows before it");
    CSTS_REQUIRE(job[OVG_WG0] == G, "a job's first workgroup is not the number of workgroups of the jobs before it");
    if (yuv) CSTS_REQUIRE(H >= 2 && W >= 2 && (H & 1) == 0 && (W & 1) == 0 && H <= 65534, "4:2:0 frames need even H, W >= 2, H <= 65534");
    if (pointers) {
      const int64_t a = job[OVG_SRC], b = job[OVG_DST], v = job[OVG_VEC];
      CSTS_REQUIRE(a != 0 && b != 0, "a job has a null source or destination");
      CSTS_REQUIRE(v == 0 || (v == 1 && (W & 3) == 0 && (a & 3) == 0 && (b & 3) == 0),
                   "a job's vector flag is set but W % 4 != 0 or its frames or out are not 4-byte aligned");
      if (yuv) CSTS_REQUIRE(v == 1, "the 4:2:0 group launch takes vector-path jobs only (W % 4 == 0, 4-byte aligned): send the job "
                                    "through csts_gaze_overlay_yuv");
    }
    P = job[OVG_ROW0] + K;
    G += K * cdiv(H, OV_ROWS);
    CSTS_REQUIRE(P < ((int64_t)1 << 31) && G < ((int64_t)1 << 31), "the frames and the workgroups of a call must stay below 2^31");
    max_w = std::max(max_w, W);
  }
  *rows = P;
  *grid = G;
  return (int)max_w;
}

// No job may write what another job reads or writes; a job may write its own frames (dst == src).  The destinations are sorted,
// so neighbours show every overlap among them, and every source is looked up among them.  bytes(job) -> the bytes of its frames.
template <typename Bytes>
int ovg_disjoint(const int64_t* jobs_host, int njobs, Bytes bytes) {
  struct Span { int64_t lo, hi; int job; };
  std::vector<Span> dst(njobs);
  for (int j = 0; j < njobs; ++j) {
    const int64_t* job = jobs_host + (int64_t)j * OVG_JOB;
    dst[j] = {job[OVG_DST], job[OVG_DST] + bytes(job), j};
  }
  std::sort(dst.begin(), dst.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
  for (int j = 1; j < njobs; ++j) CSTS_REQUIRE(dst[j - 1].hi <= dst[j].lo, "the outputs of two jobs overlap");
  for (int j = 0; j < njobs; ++j) {
    const int64_t* job = jobs_host + (int64_t)j * OVG_JOB;
    const int64_t lo = job[OVG_SRC], hi = lo + bytes(job);
    // the first destination that ends after lo; the ones behind it start at or after its end
    auto it = std::upper_bound(dst.begin(), dst.end(), lo, [](int64_t v, const Span& s) { return v < s.hi; });
    if (it != dst.end() && it->job == j && it->lo == lo) ++it;  // in place: the job's own frames
    CSTS_REQUIRE(it == dst.end() || it->lo >= hi, "a job's out overlaps frames: its own (other than in place) or another job's");
  }
  return 0;
}

// LDS spans of one row pair of a tile of tw pixels: two luma rows of *lcap bytes, then the chroma: one interleaved row (nv12) or a
// U and a V row of *ccap bytes each (i420), 2 * *ccap >= *lcap; returns the bytes of the pair
__host__ __device__ inline int ovy_pair_bytes(int tw, int* lcap, int* ccap) {
  *lcap = (tw + 30 + 15) / 16 * 16;
  *ccap = (tw / 2 + 30 + 15) / 16 * 16;
  return 2 * *lcap + 2 * *ccap;
}

// grid N * bands * xtiles, 256 threads.  src / dst: the addresses of frames / out rounded DOWN to 16 bytes, the tensors are the
// bytes [lo, hi) / from olo on; the frames are the H x W windows of the surfaces sf, out holds surfaces like them.  twn: pixels of a full tile (a multiple of 16).  Dynamic LDS: 2 OVY_BAND row entries, the JET table,
// the map, twn column entries, OVY_PAIRS source spans and OVY_PAIRS images.
__global__ __launch_bounds__(256) void gaze_overlay_yuv_kernel(const uint8_t* src, int64_t lo, int64_t hi, uint8_t* dst, int64_t olo,
                                                               const float* __restrict__ rescaled, const int* __restrict__ centers,
                                                               const int* __restrict__ params, int bands, int xtiles, int twn, int H,
                                                               int W, YuvSurf sf, int S, int mh, int mw, float alpha, int radius, int layout,
                                                               YuvCoef kf, RgbCoef kr) {
  extern __shared__ __align__(16) uint8_t lds[];
  OvRow* rows = reinterpret_cast<OvRow*>(lds);
  float* lut = reinterpret_cast<float*>(rows + 2 * OVY_BAND);
  float* map = lut + 256 * 3;                                   // 16-byte aligned
  uint2* cols = reinterpret_cast<uint2*>(map + ((mh * mw + 3) & ~3));
  int lcap, ccap;
  const int pair_bytes = ovy_pair_bytes(twn, &lcap, &ccap);
  uint8_t* in = reinterpret_cast<uint8_t*>(cols + twn);        // twn is even: 16-byte aligned
  uint8_t* img = in + OVY_PAIRS * pair_bytes;
  const int tid = threadIdx.x;
  const int xt = blockIdx.x % xtiles, band = (blockIdx.x / xtiles) % bands;
  const int64_t n = blockIdx.x / xtiles / bands;
  const int x0 = xt * twn, tw = min(twn, W - x0), ht = tw >> 1;
  const int P0 = band * OVY_BAND, npairs = min(OVY_BAND, (H >> 1) - P0);
  const bool nv12 = layout == CSTS_YUV_NV12;
  const bool in_place = src == dst && lo == olo;
  const int nspans = nv12 ? 3 : 4, cstep = nv12 ? 2 : 1;
  const OvyFrame f = ovy_frame(centers, params, n, S);
  if (!f.crop && !f.marked && in_place) return;                 // uniform: nothing of this frame is drawn
  ovy_tables(rows, lut, map, cols, rescaled + n * mh * mw, f, alpha, 2 * P0, 2 * npairs, x0, tw, H, W, S, mh, mw, tid);
  __syncthreads();

  const float oma = 1.0f - alpha;
  const int64_t fin = lo + n * yuv_frame_bytes(sf), fout = olo + n * yuv_frame_bytes(sf);
  const int base[4] = {0, lcap, 2 * lcap, 2 * lcap + ccap};    // where the four spans of a pair lie in its LDS bytes
  const int len[4] = {tw, tw, nv12 ? tw : ht, ht};
  for (int pp = 0; pp < npairs; pp += OVY_PAIRS) {
    const int nq = min(OVY_PAIRS, npairs - pp);
    OvyPair pair[OVY_PAIRS];
    bool live[OVY_PAIRS];
    int sh[OVY_PAIRS][4];                                       // where the first byte of each staged span lies in in[]
    int64_t o[OVY_PAIRS][4];                                    // where each output span starts, counted from dst
#pragma unroll
    for (int q = 0; q < OVY_PAIRS; ++q) {                       // everything about a row pair is uniform over the workgroup
      live[q] = false;
      if (q >= nq) continue;
      const int cy = P0 + pp + q;
      pair[q] = ovy_pair(rows + 2 * (pp + q), cy, f, radius);
      live[q] = !in_place || pair[q].drawn;
      if (!live[q]) continue;
      const int64_t lum = yuv_luma_row(sf, 2 * cy) + x0, chr = yuv_chroma_row(sf, cy, nv12) + (nv12 ? x0 : x0 >> 1);
      const int64_t off[4] = {lum, lum + sf.Ws, chr, chr + yuv_vplane(sf)};
      uint8_t* d = in + q * pair_bytes;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[q][k] = fout + off[k];
        if (k < nspans) sh[q][k] = base[k] + yuv_stage(d + base[k], src, fin + off[k], fin + off[k] + len[k], lo, hi, tid, 256);
      }
      if (nv12) sh[q][3] = sh[q][2] + 1;                        // V follows U
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < OVY_PAIRS; ++q) {
      if (!live[q]) continue;
      const uint8_t* s = in + q * pair_bytes;
      uint8_t* im = img + q * pair_bytes;
      int os[4];                                                // where the first byte of each output span lies in its image
#pragma unroll
      for (int k = 0; k < 4; ++k) os[k] = base[k] + (int)(o[q][k] & 15);
      if (nv12) os[3] = os[2] + 1;
      for (int b = tid; b < ht; b += 256) {
        int Y[2][2] = {{s[sh[q][0] + 2 * b], s[sh[q][0] + 2 * b + 1]}, {s[sh[q][1] + 2 * b], s[sh[q][1] + 2 * b + 1]}};
        int U = s[sh[q][2] + b * cstep], V = s[sh[q][3] + b * cstep];
        if (pair[q].drawn) ovy_block(Y, U, V, x0 + 2 * b, pair[q], cols + 2 * b, f.cX, radius, map, lut, oma, kf, kr);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          im[os[r] + 2 * b] = (uint8_t)Y[r][0];
          im[os[r] + 2 * b + 1] = (uint8_t)Y[r][1];
        }
        im[os[2] + b * cstep] = (uint8_t)U;
        im[os[3] + b * cstep] = (uint8_t)V;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < OVY_PAIRS; ++q) {
      if (!live[q]) continue;
      const uint8_t* im = img + q * pair_bytes;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = (int)(o[q][k] & 15);
        if (k < nspans) yuv_unstage(dst + (o[q][k] - b), im + base[k], b, b + len[k], tid, 256);
      }
    }
    // no barrier here: the next pass stages into in[] (last read before the barrier above) and writes img[] only after its own
    // barrier, which every thread reaches after it has finished this pass's write-back
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

extern "C" int csts_gaze_overlay_yuv_win(const uint8_t* frames_yuv, const float* rescaled, const int* centers, const int* params,
                                         uint8_t* out, int64_t N, int H, int W, int Hs, int Ws, int top, int left, int S, int mh,
                                         int mw, float alpha, int radius, int layout, int matrix, int full_range,
                                         hipStream_t stream) {
  CSTS_REQUIRE(frames_yuv && rescaled && params && out, "bad args (frames, rescaled, params and out must not be NULL)");
  CSTS_REQUIRE(yuv_args_ok(layout, matrix), "layout must be CSTS_YUV_NV12 or CSTS_YUV_I420, matrix CSTS_YUV_BT601 or CSTS_YUV_BT709");
  CSTS_REQUIRE(H >= 2 && W >= 2 && (H & 1) == 0 && (W & 1) == 0, "4:2:0 frames need even H, W >= 2");
  const YuvSurf sf = {Hs, Ws, top, left};
  CSTS_REQUIRE(yuv_surf_ok(H, W, sf), YUV_SURF_MSG);
  CSTS_REQUIRE(N >= 1 && H <= 65534 && W <= OV_MAX_W && S >= 1 && S <= 4096, "bad sizes (N >= 1, H <= 65534, W <= 8192, S <= 4096)");
  CSTS_REQUIRE(mh >= 1 && mw >= 1 && (int64_t)mh * mw <= CSTS_GAZE_DECODE_MAX_HW, "1 <= mh * mw <= CSTS_GAZE_DECODE_MAX_HW (the map is staged in LDS)");
  CSTS_REQUIRE(alpha >= 0.f && alpha <= 1.f, "0 <= alpha <= 1");
  CSTS_REQUIRE(radius >= 0, "radius >= 0");
  const int64_t fb = yuv_frame_bytes(sf);
  CSTS_REQUIRE(N <= ((int64_t)1 << 62) / fb, "bad sizes (N H W 3 / 2 overflows)");
  const int64_t bytes = N * fb;
  CSTS_REQUIRE(out == frames_yuv || frames_yuv + bytes <= out || out + bytes <= frames_yuv,
               "out must be the frames themselves (in place) or not overlap them");
  const int64_t bands = cdiv(H / 2, OVY_BAND), xtiles = cdiv(W, OVY_TW);
  CSTS_REQUIRE(N * bands * xtiles < ((int64_t)1 << 31), "N * ceil(H / 32) * ceil(W / 2048) must stay below 2^31");
  const int tables = 2 * OVY_BAND * (int)sizeof(OvRow) + 256 * 3 * (int)sizeof(float) + ((mh * mw + 3) & ~3) * (int)sizeof(float);
  const YuvCoef kf = yuv_coef(matrix, full_range);
  const RgbCoef kr = rgb_coef(matrix, full_range);
  if (out != frames_yuv && (Hs != H || Ws != W)) {
    // the bytes around the window come over as they are, and the window is then drawn in place on the copy: the same bytes
    CSTS_REQUIRE(hipMemcpyAsync(out, frames_yuv, (size_t)bytes, hipMemcpyDeviceToDevice, stream) == hipSuccess, "copying the surface");
    frames_yuv = out;
  }
  if (((W | Ws | left) & 3) == 0 && (reinterpret_cast<uintptr_t>(frames_yuv) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
    const int lds = tables + W * (int)sizeof(uint2);
    const bool nv12 = layout == CSTS_YUV_NV12;
    const void* fn = nv12 ? reinterpret_cast<const void*>(&gaze_overlay_yuv_vec_kernel<true>)
                          : reinterpret_cast<const void*>(&gaze_overlay_yuv_vec_kernel<false>);
    if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(fn, lds), "LDS opt-in");
    if (nv12) hipLaunchKernelGGL(gaze_overlay_yuv_vec_kernel<true>, dim3((unsigned)(N * bands)), dim3(256), lds, stream, frames_yuv,
                                 out, rescaled, centers, params, (int)bands, H, W, sf, S, mh, mw, alpha, radius, kf, kr);
    else hipLaunchKernelGGL(gaze_overlay_yuv_vec_kernel<false>, dim3((unsigned)(N * bands)), dim3(256), lds, stream, frames_yuv, out,
                            rescaled, centers, params, (int)bands, H, W, sf, S, mh, mw, alpha, radius, kf, kr);
    CSTS_LAUNCH_CHECK();
    return 0;
  }
  const int twn = (int)((cdiv(W, xtiles) + 15) / 16 * 16);      // an even split of the row, <= OVY_TW
  int lcap, ccap;
  const int lds = tables + twn * (int)sizeof(uint2) + 2 * OVY_PAIRS * ovy_pair_bytes(twn, &lcap, &ccap);
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&gaze_overlay_yuv_kernel), lds), "LDS opt-in");
  const int64_t lo = (int64_t)(reinterpret_cast<uintptr_t>(frames_yuv) & 15), olo = (int64_t)(reinterpret_cast<uintptr_t>(out) & 15);
  hipLaunchKernelGGL(gaze_overlay_yuv_kernel, dim3((unsigned)(N * bands * xtiles)), dim3(256), lds, stream, frames_yuv - lo, lo,
                     lo + bytes, out - olo, olo, rescaled, centers, params, (int)bands, (int)xtiles, twn, H, W, sf, S, mh, mw, alpha,
                     radius, layout, kf, kr);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_gaze_overlay_yuv(const uint8_t* frames_yuv, const float* rescaled, const int* centers, const int* params,
                                     uint8_t* out, int64_t N, int H, int W, int S, int mh, int mw, float alpha, int radius, int layout,
                                     int matrix, int full_range, hipStream_t stream) {
  return csts_gaze_overlay_yuv_win(frames_yuv, rescaled, centers, params, out, N, H, W, H, W, 0, 0, S, mh, mw, alpha, radius, layout,
                                   matrix, full_range, stream);
}

extern "C" int csts_group_gaze_overlay(const int64_t* jobs, const int64_t* jobs_host, int njobs, const float* rescaled,
                                       const int* centers, int S, int mh, int mw, float alpha, int radius, hipStream_t stream) {
  int64_t rows, grid;
  const int max_w = ovg_check(jobs_host, njobs, false, true, &rows, &grid);
  if (max_w < 0) return -1;
  CSTS_REQUIRE(jobs && rescaled, "bad args (jobs and rescaled must not be NULL)");
  CSTS_REQUIRE(S >= 1 && S <= 4096, "bad sizes (1 <= S <= 4096)");
  CSTS_REQUIRE(mh >= 1 && mw >= 1 && (int64_t)mh * mw <= CSTS_GAZE_DECODE_MAX_HW, "1 <= mh * mw <= CSTS_GAZE_DECODE_MAX_HW (the map is staged in LDS)");
  CSTS_REQUIRE(alpha >= 0.f && alpha <= 1.f, "0 <= alpha <= 1");
  CSTS_REQUIRE(radius >= 0, "radius >= 0");
  if (ovg_disjoint(jobs_host, njobs, [](const int64_t* job) { return job[OVG_K] * job[OVG_H] * job[OVG_W] * 3; })) return -1;
  const int lds = OV_ROWS * (int)sizeof(OvRow) + 256 * 3 * (int)sizeof(float) + ((mh * mw + 1) & ~1) * (int)sizeof(float) + max_w * (int)sizeof(uint2);
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&group_gaze_overlay_kernel), lds), "LDS opt-in");
  hipLaunchKernelGGL(group_gaze_overlay_kernel, dim3((unsigned)grid), dim3(256), lds, stream, jobs, njobs, max_w, rescaled, centers, S,
                     mh, mw, alpha, radius);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_group_gaze_overlay_yuv(const int64_t* jobs, const int64_t* jobs_host, int njobs, const float* rescaled,
                                           const int* centers, int S, int mh, int mw, float alpha, int radius, int layout, int matrix,
                                           int full_range, hipStream_t stream) {
  CSTS_REQUIRE(yuv_args_ok(layout, matrix), "layout must be CSTS_YUV_NV12 or CSTS_YUV_I420, matrix CSTS_YUV_BT601 or CSTS_YUV_BT709");
  int64_t rows, grid;
  const int max_w = ovg_check(jobs_host, njobs, true, true, &rows, &grid);
  if (max_w < 0) return -1;
  CSTS_REQUIRE(jobs && rescaled, "bad args (jobs and rescaled must not be NULL)");
  CSTS_REQUIRE(S >= 1 && S <= 4096, "bad sizes (1 <= S <= 4096)");
  CSTS_REQUIRE(mh >= 1 && mw >= 1 && (int64_t)mh * mw <= CSTS_GAZE_DECODE_MAX_HW, "1 <= mh * mw <= CSTS_GAZE_DECODE_MAX_HW (the map is staged in LDS)");
  CSTS_REQUIRE(alpha >= 0.f && alpha <= 1.f, "0 <= alpha <= 1");
  CSTS_REQUIRE(radius >= 0, "radius >= 0");
  if (ovg_disjoint(jobs_host, njobs, [](const int64_t* job) { return job[OVG_K] * yuv_frame_bytes((int)job[OVG_H], (int)job[OVG_W]); }))
    return -1;
  const int lds = 2 * OVY_BAND * (int)sizeof(OvRow) + 256 * 3 * (int)sizeof(float) + ((mh * mw + 3) & ~3) * (int)sizeof(float) +
                  max_w * (int)sizeof(uint2);
  const YuvCoef kf = yuv_coef(matrix, full_range);
  const RgbCoef kr = rgb_coef(matrix, full_range);
  const bool nv12 = layout == CSTS_YUV_NV12;
  const void* fn = nv12 ? reinterpret_cast<const void*>(&group_gaze_overlay_yuv_kernel<true>)
                        : reinterpret_cast<const void*>(&group_gaze_overlay_yuv_kernel<false>);
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(fn, lds), "LDS opt-in");
  if (nv12) hipLaunchKernelGGL(group_gaze_overlay_yuv_kernel<true>, dim3((unsigned)grid), dim3(256), lds, stream, jobs, njobs, max_w,
                               rescaled, centers, S, mh, mw, alpha, radius, kf, kr);
  else hipLaunchKernelGGL(group_gaze_overlay_yuv_kernel<false>, dim3((unsigned)grid), dim3(256), lds, stream, jobs, njobs, max_w, rescaled,
                          centers, S, mh, mw, alpha, radius, kf, kr);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_group_points_source(const int64_t* jobs, const int64_t* jobs_host, int njobs, const float* points, int S,
                                        double* points_source, int* centers, hipStream_t stream) {
  int64_t rows, grid;
  if (ovg_check(jobs_host, njobs, false, false, &rows, &grid) < 0) return -1;
  CSTS_REQUIRE(jobs && points && points_source && centers, "bad args (jobs, points, points_source and centers must not be NULL)");
  CSTS_REQUIRE(S >= 1 && S <= 4096, "bad sizes (1 <= S <= 4096)");
  for (int j = 0; j < njobs; ++j) {
    const int64_t* job = jobs_host + (int64_t)j * OVG_JOB;
    CSTS_REQUIRE(job[OVG_NH] >= 1 && job[OVG_NW] >= 1 && job[OVG_NH] <= (1 << 24) && job[OVG_NW] <= (1 << 24) && job[OVG_Y0] >= 0 &&
                     job[OVG_X0] >= 0 && job[OVG_Y0] <= (1 << 24) && job[OVG_X0] <= (1 << 24),
                 "a job's params row is out of range (1 <= new h, new w <= 2^24, 0 <= y0, x0 <= 2^24)");
  }
  hipLaunchKernelGGL(group_points_source_kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0, stream, jobs, njobs, points,
                     points_source, centers, rows, S);
  CSTS_LAUNCH_CHECK();
  return 0;
}
