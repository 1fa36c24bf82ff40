// What the gaze-track kernels share (decode.hip: gaze_decode, gaze_track, gaze_track_fill; stream.hip: live_track_rows): the
// register layout of one frame's map over a workgroup of 256 lanes, the (max, arg-max) rule, the tail that turns a map into
// heatmaps / rescaled / points / peak, and the time-linear blend of two maps.  One device function each, so a map that went
// through the same rule leaves every kernel with the same bits.
#pragma once
#include "common.h"

namespace {

constexpr int DEC_MAX_NCH = CSTS_GAZE_DECODE_MAX_HW / 1024;      // 4-value chunks per lane at the largest frame

// Element r of chunk c of lane tid.  VEC: 4 consecutive cells per chunk (128-bit stores, 64- / 128-bit loads); otherwise the
// cells of a chunk are 256 apart (frames whose size or address does not allow vector access).
template <bool VEC>
__device__ __forceinline__ int cell_of(int c, int r, int tid) {
  return VEC ? (c * 256 + tid) * 4 + r : (c * 4 + r) * 256 + tid;
}

// (value, index) pair with "larger value wins, lowest index on ties"
__device__ __forceinline__ void take_max(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// The tail gaze_track, gaze_track_fill and live_track_rows share: the frame's map m (registers, layout of cell_of) -> its max +
// arg-max (a lane walks its cells in ascending index order) and its min, then heatmaps = m, rescaled, points and peak of frame
// blockIdx.x.  live = false (nobody predicts the frame; the caller passes m = 0): maps 0, points NaN, peak 0.
template <int NCH, bool VEC>
__device__ __forceinline__ void track_tail(const float (&m)[NCH * 4], bool live, int H, int W, float* __restrict__ heatmaps,
                                           float* __restrict__ rescaled, float* __restrict__ points, float* __restrict__ peak) {
  __shared__ float red_v[2][4];
  __shared__ int red_i[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int hw = H * W;
  const int64_t frame = blockIdx.x, base = frame * hw;
  float bv = -INFINITY, mn = INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int at = cell_of<VEC>(c, r, tid);
      if (at < hw) {
        take_max(bv, bi, m[c * 4 + r], at);
        mn = fminf(mn, m[c * 4 + r]);
      }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) take_max(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
  mn = -wave_max(-mn);
  if (lane == 0) { red_v[0][w] = bv; red_i[w] = bi; red_v[1][w] = mn; }
  __syncthreads();
  bv = red_v[0][0]; bi = red_i[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) take_max(bv, bi, red_v[0][k], red_i[k]);
  if (bi >= hw) bi = 0;                 // a frame without a comparable value (all NaN): still a cell of the frame
  mn = fminf(fminf(red_v[1][0], red_v[1][1]), fminf(red_v[1][2], red_v[1][3]));
  const float denom = bv - mn + 1e-6f;
  // ---- writes (an uncovered frame: m = 0 everywhere, so the maps below are 0)
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (VEC) {
      const int at = (c * 256 + tid) * 4;
      if (at < hw) {
        f32x4 p, q;
#pragma unroll
        for (int r = 0; r < 4; ++r) { p[r] = m[c * 4 + r]; q[r] = (p[r] - mn) / denom; }
        if (heatmaps) *reinterpret_cast<f32x4*>(heatmaps + base + at) = p;
        if (rescaled) *reinterpret_cast<f32x4*>(rescaled + base + at) = q;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = cell_of<false>(c, r, tid);
        if (at < hw) {
          if (heatmaps) heatmaps[base + at] = m[c * 4 + r];
          if (rescaled) rescaled[base + at] = (m[c * 4 + r] - mn) / denom;
        }
      }
    }
  }
  if (tid == 0) {
    if (points) {
      const int row = bi / W, col = bi - row * W;
      points[frame * 2] = live ? (float)col / (float)W : __builtin_nanf("");
      points[frame * 2 + 1] = live ? (float)row / (float)H : __builtin_nanf("");
    }
    if (peak) peak[frame] = live ? bv : 0.f;
  }
}

// One map row -> registers in the layout of cell_of; cells past the frame are 0.
template <int NCH, bool VEC>
__device__ __forceinline__ void load_map(float (&m)[NCH * 4], const float* __restrict__ row, int hw, int tid) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (VEC) {
      const int at = (c * 256 + tid) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (at < hw) v = *reinterpret_cast<const f32x4*>(row + at);       // hw % 4 == 0 on this path
#pragma unroll
      for (int r = 0; r < 4; ++r) m[c * 4 + r] = v[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = cell_of<false>(c, r, tid);
        m[c * 4 + r] = at < hw ? row[at] : 0.f;
      }
    }
  }
}

// The time-linear blend of frame n between its neighbours a < n < b: m = wa * m + wb * hb, two products and one sum in fp32
// (the library is built without contraction), wa = (b - n) / (b - a), wb = (n - a) / (b - a).  Factored out of gaze_fill_kernel:
// the frame numbers are int64 here (a live stream has no last frame) where that kernel had int; the same fp32 values.
template <int NCH>
__device__ __forceinline__ void blend_maps(float (&m)[NCH * 4], const float (&hb)[NCH * 4], int64_t a, int64_t b, int64_t n) {
  const float span = (float)(b - a);
  const float wa = (float)(b - n) / span, wb = (float)(n - a) / span;
#pragma unroll
  for (int k = 0; k < NCH * 4; ++k) m[k] = wa * m[k] + wb * hb[k];
}

}  // namespace
