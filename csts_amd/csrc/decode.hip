// Gaze head of the inference path: everything a consumer of a prediction needs from one read of a frame's logits.
// frame_softmax (slowfast/utils/utils.py:5-12, temperature 2 on this path), the per-frame min-max rescale of the test driver
// (tools/test_avgaze_net.py:68-70), the gaze point = the arg-max cell mapped back by the inverse of the centre rule of
// _get_gaussian_map (ego4d_avgaze_forecast.py:404-407) and the peak probability.  include/csts_hip.h states the rule.
// One workgroup of 256 lanes per frame; the frame stays in registers (NCH x 4 values per lane) between the three reductions
// (max + arg-max together, exp-sum, min) and the writes, so the logits are read once and nothing is re-read from memory.
//
// gaze_track: the per-frame track of a whole video from the per-window heat maps above.  Windows that overlap predict the same
// video frame several times; the track is the mean heat map per frame, decoded again (rescale, arg-max point, peak).  One
// workgroup per OUTPUT frame walks the list of prediction rows that target it and keeps the running sum in registers in the
// layout of gaze_decode, so every row is read once, nothing is re-read and no atomics are needed: the sum has one fixed order.
#include "track_shared.h"

namespace {

template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void gaze_decode_kernel(const void* __restrict__ logits, int dt, int H, int W, float inv_temp,
                                                          float* __restrict__ preds, float* __restrict__ rescaled,
                                                          float* __restrict__ points, float* __restrict__ peak) {
  __shared__ float red_v[3][4];
  __shared__ int red_i[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int hw = H * W;
  const int64_t frame = blockIdx.x, base = frame * hw;
  float x[NCH * 4];                     // logits, then exp(logit / temperature - max)
  // ---- one read of the frame
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (VEC) {
      const int at = (c * 256 + tid) * 4;
      if (at < hw) {                    // hw % 4 == 0 on this path: a chunk is inside the frame or outside it
        if (dt == CSTS_F32) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(logits) + base + at);
#pragma unroll
          for (int r = 0; r < 4; ++r) x[c * 4 + r] = v[r];
        } else {
          const bf16x4 v = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(logits) + base + at);
#pragma unroll
          for (int r = 0; r < 4; ++r) x[c * 4 + r] = (float)v[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) x[c * 4 + r] = -INFINITY;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = cell_of<false>(c, r, tid);
        x[c * 4 + r] = at < hw ? ld_as_f32(logits, dt, base + at) : -INFINITY;
      }
    }
  }
  // ---- max and arg-max of the logits together (the softmax is monotone: this is the heat map's maximum; a lane walks its
  // cells in ascending index order, so `>` keeps the lowest index)
  float bv = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int at = cell_of<VEC>(c, r, tid);
      if (at < hw) take_max(bv, bi, x[c * 4 + r], at);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) take_max(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
  if (lane == 0) { red_v[0][w] = bv; red_i[w] = bi; }
  __syncthreads();
  bv = red_v[0][0]; bi = red_i[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) take_max(bv, bi, red_v[0][k], red_i[k]);
  if (bi >= hw) bi = 0;                 // a frame without a comparable value (all NaN): still a cell of the frame
  const float mx = bv * inv_temp;       // = max of logit * inv_temp (inv_temp > 0)
  // ---- exp-sum and min (cells outside the frame hold exp(-inf) = 0 and are kept out of the min)
  float s = 0.f, emin = INFINITY;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __expf(x[c * 4 + r] * inv_temp - mx);
      x[c * 4 + r] = e;
      s += e;
      if (cell_of<VEC>(c, r, tid) < hw) emin = fminf(emin, e);
    }
  s = wave_sum(s);
  if (lane == 0) red_v[1][w] = s;
  __syncthreads();
  s = red_v[1][0] + red_v[1][1] + red_v[1][2] + red_v[1][3];
  emin = -wave_max(-emin);
  if (lane == 0) red_v[2][w] = emin;
  __syncthreads();
  emin = fminf(fminf(red_v[2][0], red_v[2][1]), fminf(red_v[2][2], red_v[2][3]));
  const float inv = 1.f / s;
  const float pmax = __expf(bv * inv_temp - mx) * inv;      // the arg-max cell's probability (exp(0) = 1)
  const float pmin = emin * inv;                            // min of e * inv: the product is monotone in e
  const float denom = pmax - pmin + 1e-6f;
  // ---- writes
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (VEC) {
      const int at = (c * 256 + tid) * 4;
      if (at < hw) {
        f32x4 p, q;
#pragma unroll
        for (int r = 0; r < 4; ++r) { p[r] = x[c * 4 + r] * inv; q[r] = (p[r] - pmin) / denom; }
        if (preds) *reinterpret_cast<f32x4*>(preds + base + at) = p;
        if (rescaled) *reinterpret_cast<f32x4*>(rescaled + base + at) = q;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = cell_of<false>(c, r, tid);
        if (at < hw) {
          const float p = x[c * 4 + r] * inv;
          if (preds) preds[base + at] = p;
          if (rescaled) rescaled[base + at] = (p - pmin) / denom;
        }
      }
    }
  }
  if (tid == 0) {
    if (points) {
      const int row = bi / W, col = bi - row * W;
      points[frame * 2] = (float)col / (float)W;
      points[frame * 2 + 1] = (float)row / (float)H;
    }
    if (peak) peak[frame] = pmax;
  }
}

template <int NCH>
void launch_decode(bool vec, unsigned nframes, hipStream_t stream, const void* logits, int dt, int H, int W, float inv_temp,
                   float* preds, float* rescaled, float* points, float* peak) {
  if (vec) hipLaunchKernelGGL((gaze_decode_kernel<NCH, true>), dim3(nframes), dim3(256), 0, stream, logits, dt, H, W, inv_temp, preds,
                              rescaled, points, peak);
  else hipLaunchKernelGGL((gaze_decode_kernel<NCH, false>), dim3(nframes), dim3(256), 0, stream, logits, dt, H, W, inv_temp, preds,
                          rescaled, points, peak);
}

// One workgroup per output frame f: order[offsets[f] .. offsets[f + 1]) are its prediction rows, added in that order.
template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void gaze_track_kernel(const float* __restrict__ preds, const int* __restrict__ order,
                                                         const int* __restrict__ offsets, int H, int W,
                                                         float* __restrict__ heatmaps, float* __restrict__ rescaled,
                                                         float* __restrict__ points, float* __restrict__ peak,
                                                         int* __restrict__ count) {
  const int tid = threadIdx.x;
  const int hw = H * W;
  const int64_t frame = blockIdx.x;
  const int beg = offsets[frame], n = offsets[frame + 1] - beg;          // uniform over the workgroup
  float m[NCH * 4];
#pragma unroll
  for (int k = 0; k < NCH * 4; ++k) m[k] = 0.f;
  for (int j = 0; j < n; ++j) {
    const float* row = preds + (int64_t)order[beg + j] * hw;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (VEC) {
        const int at = (c * 256 + tid) * 4;
        if (at < hw) {                  // hw % 4 == 0 on this path: a chunk is inside the frame or outside it
          const f32x4 v = *reinterpret_cast<const f32x4*>(row + at);
#pragma unroll
          for (int r = 0; r < 4; ++r) m[c * 4 + r] += v[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int at = cell_of<false>(c, r, tid);
          if (at < hw) m[c * 4 + r] += row[at];
        }
      }
    }
  }
  const float inv = n > 0 ? 1.f / (float)n : 0.f;
#pragma unroll
  for (int k = 0; k < NCH * 4; ++k) m[k] *= inv;
  track_tail<NCH, VEC>(m, n > 0, H, W, heatmaps, rescaled, points, peak);
  if (tid == 0 && count) count[frame] = n;
}

template <int NCH>
void launch_track(bool vec, unsigned nframes, hipStream_t stream, const float* preds, const int* order, const int* offsets, int H,
                  int W, float* heatmaps, float* rescaled, float* points, float* peak, int* count) {
  if (vec) hipLaunchKernelGGL((gaze_track_kernel<NCH, true>), dim3(nframes), dim3(256), 0, stream, preds, order, offsets, H, W,
                              heatmaps, rescaled, points, peak, count);
  else hipLaunchKernelGGL((gaze_track_kernel<NCH, false>), dim3(nframes), dim3(256), 0, stream, preds, order, offsets, H, W,
                          heatmaps, rescaled, points, peak, count);
}

// gaze_track_fill: one workgroup per output frame n.  A predicted frame (count[n] > 0) passes through; any other frame looks
// for its nearest predicted neighbours a < n < b itself, at most max_gap - 1 frames each way (count is read at wave-uniform
// addresses), and takes H_a (hold) or wa H_a + wb H_b (linear) when b - a <= max_gap.  The map then goes through track_tail,
// so a predicted frame leaves with the bits gaze_track wrote for it.
template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void gaze_fill_kernel(const float* __restrict__ maps, const int* __restrict__ count, int F, int H,
                                                        int W, int mode, int max_gap, float* __restrict__ heatmaps,
                                                        float* __restrict__ rescaled, float* __restrict__ points,
                                                        float* __restrict__ peak, int* __restrict__ neighbours) {
  const int tid = threadIdx.x;
  const int hw = H * W;
  const int n = blockIdx.x;                                               // uniform over the workgroup, as a, b below
  int a = -1, b = -1;
  if (count[n] > 0) {
    a = b = n;
  } else {
    const int lo = max(n - (max_gap - 1), 0);
    for (int j = n - 1; j >= lo; --j)
      if (count[j] > 0) { a = j; break; }
    if (a >= 0) {
      const int hi = (int)min((int64_t)a + max_gap, (int64_t)F - 1);     // b - a <= max_gap
      for (int j = n + 1; j <= hi; ++j)
        if (count[j] > 0) { b = j; break; }
    }
    if (b < 0) a = -1;
  }
  float m[NCH * 4];
  if (a < 0) {
#pragma unroll
    for (int k = 0; k < NCH * 4; ++k) m[k] = 0.f;
  } else {
    load_map<NCH, VEC>(m, maps + (int64_t)a * hw, hw, tid);
    if (mode == 1 && b != a) {
      float hb[NCH * 4];
      load_map<NCH, VEC>(hb, maps + (int64_t)b * hw, hw, tid);
      blend_maps<NCH>(m, hb, a, b, n);
    }
  }
  track_tail<NCH, VEC>(m, a >= 0, H, W, heatmaps, rescaled, points, peak);
  if (tid == 0 && neighbours) { neighbours[2 * (int64_t)n] = a; neighbours[2 * (int64_t)n + 1] = b; }
}

template <int NCH>
void launch_fill(bool vec, unsigned nframes, hipStream_t stream, const float* maps, const int* count, int H, int W, int mode,
                 int max_gap, float* heatmaps, float* rescaled, float* points, float* peak, int* neighbours) {
  if (vec) hipLaunchKernelGGL((gaze_fill_kernel<NCH, true>), dim3(nframes), dim3(256), 0, stream, maps, count, (int)nframes, H, W,
                              mode, max_gap, heatmaps, rescaled, points, peak, neighbours);
  else hipLaunchKernelGGL((gaze_fill_kernel<NCH, false>), dim3(nframes), dim3(256), 0, stream, maps, count, (int)nframes, H, W,
                          mode, max_gap, heatmaps, rescaled, points, peak, neighbours);
}

}  // namespace

extern "C" int csts_gaze_decode(const void* logits, int dt, int64_t nframes, int H, int W, float temperature, float* preds,
                                float* rescaled, float* points, float* peak, hipStream_t stream) {
  CSTS_REQUIRE(logits, "null logits");
  CSTS_REQUIRE(dt == CSTS_F32 || dt == CSTS_BF16, "logits must be fp32 or the library's 16-bit type");
  CSTS_REQUIRE(nframes >= 1 && nframes < ((int64_t)1 << 31), "1 <= frames < 2^31");
  CSTS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= CSTS_GAZE_DECODE_MAX_HW, "1 <= H * W <= CSTS_GAZE_DECODE_MAX_HW (the frame is held in registers)");
  CSTS_REQUIRE(temperature > 0.f, "temperature must be positive");
  if (!preds && !rescaled && !points && !peak) return 0;
  const int hw = H * W;
  const bool vec = hw % 4 == 0 && aligned16(logits) && aligned16(preds) && aligned16(rescaled);
  const int nch = (int)cdiv(hw, 1024);
  static_assert(DEC_MAX_NCH == 8, "the dispatch below covers 1, 2, 4 and 8 chunks per lane");
  const unsigned n = (unsigned)nframes;
  const float it = 1.f / temperature;
  if (nch <= 1) launch_decode<1>(vec, n, stream, logits, dt, H, W, it, preds, rescaled, points, peak);
  else if (nch <= 2) launch_decode<2>(vec, n, stream, logits, dt, H, W, it, preds, rescaled, points, peak);
  else if (nch <= 4) launch_decode<4>(vec, n, stream, logits, dt, H, W, it, preds, rescaled, points, peak);
  else launch_decode<8>(vec, n, stream, logits, dt, H, W, it, preds, rescaled, points, peak);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_gaze_track(const float* preds, const int* order, const int* offsets, int64_t F, int H, int W, float* heatmaps,
                               float* rescaled, float* points, float* peak, int* count, hipStream_t stream) {
  CSTS_REQUIRE(preds && order && offsets, "null preds, order or offsets");
  CSTS_REQUIRE(F >= 1 && F < ((int64_t)1 << 31), "1 <= frames < 2^31");
  CSTS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= CSTS_GAZE_DECODE_MAX_HW, "1 <= H * W <= CSTS_GAZE_DECODE_MAX_HW (the frame is held in registers)");
  if (!heatmaps && !rescaled && !points && !peak && !count) return 0;
  const int hw = H * W;
  const bool vec = hw % 4 == 0 && aligned16(preds) && aligned16(heatmaps) && aligned16(rescaled);
  const int nch = (int)cdiv(hw, 1024);
  const unsigned n = (unsigned)F;
  if (nch <= 1) launch_track<1>(vec, n, stream, preds, order, offsets, H, W, heatmaps, rescaled, points, peak, count);
  else if (nch <= 2) launch_track<2>(vec, n, stream, preds, order, offsets, H, W, heatmaps, rescaled, points, peak, count);
  else if (nch <= 4) launch_track<4>(vec, n, stream, preds, order, offsets, H, W, heatmaps, rescaled, points, peak, count);
  else launch_track<8>(vec, n, stream, preds, order, offsets, H, W, heatmaps, rescaled, points, peak, count);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_gaze_track_fill(const float* heatmaps, const int* count, int64_t F, int H, int W, int mode, int max_gap,
                                    float* out_heatmaps, float* out_rescaled, float* out_points, float* out_peak,
                                    int* out_neighbours, hipStream_t stream) {
  CSTS_REQUIRE(heatmaps && count, "null heatmaps or count");
  CSTS_REQUIRE(F >= 1 && F < ((int64_t)1 << 31), "1 <= frames < 2^31");
  CSTS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= CSTS_GAZE_DECODE_MAX_HW, "1 <= H * W <= CSTS_GAZE_DECODE_MAX_HW (the frame is held in registers)");
  CSTS_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (hold) or 1 (linear)");
  CSTS_REQUIRE(max_gap >= 1 && max_gap <= CSTS_GAZE_FILL_MAX_GAP, "1 <= max_gap <= CSTS_GAZE_FILL_MAX_GAP");
  CSTS_REQUIRE(out_heatmaps != heatmaps && out_rescaled != heatmaps && (const void*)out_points != (const void*)heatmaps &&
                   (const void*)out_peak != (const void*)heatmaps && (const void*)out_neighbours != (const void*)heatmaps,
               "no output may be heatmaps (a frame reads its neighbours' maps)");
  if (!out_heatmaps && !out_rescaled && !out_points && !out_peak && !out_neighbours) return 0;
  const int hw = H * W;
  const bool vec = hw % 4 == 0 && aligned16(heatmaps) && aligned16(out_heatmaps) && aligned16(out_rescaled);
  const int nch = (int)cdiv(hw, 1024);
  const unsigned n = (unsigned)F;
  if (nch <= 1) launch_fill<1>(vec, n, stream, heatmaps, count, H, W, mode, max_gap, out_heatmaps, out_rescaled, out_points, out_peak, out_neighbours);
  else if (nch <= 2) launch_fill<2>(vec, n, stream, heatmaps, count, H, W, mode, max_gap, out_heatmaps, out_rescaled, out_points, out_peak, out_neighbours);
  else if (nch <= 4) launch_fill<4>(vec, n, stream, heatmaps, count, H, W, mode, max_gap, out_heatmaps, out_rescaled, out_points, out_peak, out_neighbours);
  else launch_fill<8>(vec, n, stream, heatmaps, count, H, W, mode, max_gap, out_heatmaps, out_rescaled, out_points, out_peak, out_neighbours);
  CSTS_LAUNCH_CHECK();
  return 0;
}
