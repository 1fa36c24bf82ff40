// What spatial.hip (one clip size per call) and batch.hip (clips of many recordings, one size each) share: the rule of the spatial
// sampling, its variates, and the pixel pass of one output row.  include/csts_hip.h states the rule; spatial.hip tells the story.
#pragma once
#include "common.h"
#include "philox.h"

namespace {

constexpr uint32_t SPATIAL_STREAM = 0x53504154u;     // "SPAT": the third counter word of the spatial variates
constexpr int SPATIAL_MAX_T = 64;
constexpr int SAMPLE_ROWS = 4;                        // output rows per workgroup, one per wave

struct SpatialRule {
  int T, L, H, W, S, min_scale, max_scale, spatial_idx, random_flip, inv_uniform;
};

// u[0..3] of clip `clip`: Philox4x32-10 blocks on the counters (lo32(clip), hi32(clip), SPATIAL_STREAM, 0 | 1), two 53-bit
// doubles per block
__host__ __device__ __forceinline__ void spatial_uniforms(uint32_t k0, uint32_t k1, uint64_t clip, double u[4]) {
  for (int j = 0; j < 2; ++j) {
    uint32_t w[4] = {(uint32_t)clip, (uint32_t)(clip >> 32), SPATIAL_STREAM, (uint32_t)j};
    csts_philox::philox4x32_10(w, k0, k1);
    u[2 * j] = csts_philox::uniform53(w[0], w[1]);
    u[2 * j + 1] = csts_philox::uniform53(w[2], w[3]);
  }
}

// Python's max(0, v) / min(a, v) (the first argument unless the second is strictly larger / smaller)
__host__ __device__ __forceinline__ double py_max0(double v) { return v > 0.0 ? v : 0.0; }
__host__ __device__ __forceinline__ double py_min(double a, double v) { return v < a ? v : a; }

// random_crop_gaze along one axis of extent E > S: keep as many gaze points inside the window as the drop-one-end loop allows
__host__ __device__ inline int gaze_axis_offset(const double* lab, int col, int T, int L, int E, int S, double u, double* g) {
  if (E <= S) return 0;
  for (int t = 0; t < T; ++t) {
    const double v = lab[(int64_t)t * L + col] * (double)E;
    int k = t;
    for (; k > 0 && g[k - 1] > v; --k) g[k] = g[k - 1];     // insertion sort, ascending (T <= 64)
    g[k] = v;
  }
  const double es = (double)(E - S);
  int lo = 0, hi = T - 1;
  double low = py_max0(g[hi] - (double)S), high = py_min(es, g[lo]);
  while (low > high) {
    // one point left outside [0, E]: the reference would take max() of an empty array; the window nearest to it is taken
    if (lo == hi) return (int)py_min(es, low);
    if (((hi - lo + 1) & 1) == 0) ++lo; else --hi;
    low = py_max0(g[hi] - (double)S);
    high = py_min(es, g[lo]);
  }
  return low == high ? (int)low : (int)(low + (high - low) * u);
}

// the rule of one clip: lab (T, L) -> par {new h, new w, y0, x0, flip}, out (T, L); g: T doubles of scratch
__host__ __device__ inline void spatial_rule(const double* lab, const SpatialRule& a, const double u[4], int par[5], double* out,
                                             double* g) {
  const int H = a.H, W = a.W, S = a.S;
  const bool train = a.spatial_idx < 0;
  int size = S;
  if (train) {
    double v;
    if (a.inv_uniform) {
      const double lo = 1.0 / (double)a.max_scale, hi = 1.0 / (double)a.min_scale;
      v = 1.0 / (lo + (hi - lo) * u[0]);
    } else {
      v = (double)a.min_scale + ((double)a.max_scale - (double)a.min_scale) * u[0];
    }
    size = (int)rint(v);                                   // Python round(): half to even
  }
  int nh = H, nw = W;
  if (!((W <= H && W == size) || (H <= W && H == size))) {
    if (W < H) {
      nw = size;
      nh = (int)floor((double)H / (double)W * (double)size);
    } else {
      nh = size;
      nw = (int)floor((double)W / (double)H * (double)size);
    }
  }
  int y0, x0;
  bool clip = true;
  if (train) {
    if (nh == S && nw == S) {
      y0 = x0 = 0;
      clip = false;                                        // random_crop_gaze returns the labels untouched
    } else {
      x0 = gaze_axis_offset(lab, 0, a.T, a.L, nw, S, u[1], g);
      y0 = gaze_axis_offset(lab, 1, a.T, a.L, nh, S, u[2], g);
    }
  } else {
    y0 = (nh - S + 1) / 2;                                 // ceil((E - S) / 2)
    x0 = (nw - S + 1) / 2;
    if (nh > nw) {
      if (a.spatial_idx == 0) y0 = 0;
      else if (a.spatial_idx == 2) y0 = nh - S;
    } else {
      if (a.spatial_idx == 0) x0 = 0;
      else if (a.spatial_idx == 2) x0 = nw - S;
    }
  }
  const int flip = (train && a.random_flip && u[3] < 0.5) ? 1 : 0;
  for (int t = 0; t < a.T; ++t) {
    for (int l = 0; l < a.L; ++l) {
      double v = lab[(int64_t)t * a.L + l];
      if (clip && l < 2) {
        v = (v * (double)(l == 0 ? nw : nh) - (double)(l == 0 ? x0 : y0)) / (double)S;
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);           // np.clip (NaN stays NaN)
      }
      if (flip && l == 0) v = 1.0 - v;
      out[(int64_t)t * a.L + l] = v;
    }
  }
  par[0] = nh; par[1] = nw; par[2] = y0; par[3] = x0; par[4] = flip;
}

// the pixel pass of one workgroup: SAMPLE_ROWS output rows (one per wave) of frame t of clip b.  The frame is frame number `frame`
// of a recording of H x W frames that starts at byte `base` of src (src_bytes long: nothing past it is read); par = the clip's
// {new h, new w, y0, x0, flip}; bad: the caller refuses the recording (NaN clip).  Every thread of the workgroup calls it with the
// same arguments (it holds a barrier); lds: SAMPLE_ROWS x 2 x rowcap bytes, rowcap >= 3 W + 30 rounded up to 16.
__device__ __forceinline__ void sample_rows(const uint8_t* __restrict__ src, int64_t src_bytes, int64_t base, int64_t frame, int H,
                                            int W, const int* __restrict__ par, bool bad, float* __restrict__ out, int b, int t,
                                            int T, int S, int rowcap, float3 mean, float3 inv_std, uint8_t* lds) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * SAMPLE_ROWS + wv;                 // output row of this wave
  const int nh = par[0], nw = par[1], y0 = par[2], x0 = par[3], flip = par[4];
  const int64_t plane = (int64_t)S * S;
  float* o0 = out + ((int64_t)b * 3 * T + t) * plane + (int64_t)i * S;      // channel c at o0 + c * T * plane
  const int64_t cstride = (int64_t)T * plane;
  const bool row_ok = i < S;
  // parameters outside the rule's range (injected by a caller) or a refused recording: the clip's output is NaN, no pixel is read
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
  uint8_t* rows = lds + wv * 2 * rowcap;
  // the source frame: a recording starts at any byte `base` of src and a frame of H * W * 3 bytes at any byte of it, so the
  // 16-byte chunks below are laid out from the byte offset in src (16-byte aligned itself), never from the offset inside the frame
  int shift[2];
  for (int r = 0; r < 2; ++r) {
    const int64_t row0 = base + (frame * H + (r ? yb : ya)) * W * 3;
    const int64_t beg = row0 + (int64_t)xlo * 3, end = row0 + (int64_t)(xhi + 1) * 3;
    const int64_t a0 = beg & ~(int64_t)15, nbytes = ((end + 15) & ~(int64_t)15) - a0;    // <= 3 W + 30 <= rowcap
    shift[r] = (int)(beg - a0);
    if (!row_ok) continue;
    uint8_t* dst = rows + r * rowcap;
    for (int64_t k = lane * 16; k < nbytes; k += 64 * 16) {
      const int64_t g = a0 + k;
      if (g + 16 <= src_bytes) {
        *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + g);
      } else {
        for (int q = 0; q < 16; ++q) dst[k + q] = g + q < src_bytes ? src[g + q] : 0;
      }
    }
  }
  __syncthreads();
  if (!row_ok) return;
  const int ra = shift[0] - xlo * 3, rb = rowcap + shift[1] - xlo * 3;     // LDS byte of pixel x of each row: r* + 3 x
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
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p = (float)rows[ra + xa * 3 + c] * w0 + (float)rows[ra + xb * 3 + c] * w1;
        const float n = (float)rows[rb + xa * 3 + c] * w0 + (float)rows[rb + xb * 3 + c] * w1;
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

inline int spatial_check(int B, int T, int L, int H, int W, int S, int min_scale, int max_scale, int spatial_idx) {
  CSTS_REQUIRE(B > 0 && T > 0 && T <= SPATIAL_MAX_T && L >= 2, "B >= 1, 1 <= T <= 64, L >= 2 label columns");
  CSTS_REQUIRE(H > 0 && W > 0 && S > 0 && S <= 4096, "bad frame or crop size");
  CSTS_REQUIRE(spatial_idx >= -1 && spatial_idx <= 2, "spatial_idx must be -1 (train) or 0, 1, 2 (test)");
  CSTS_REQUIRE((double)std::max(H, W) / (double)std::min(H, W) * (double)std::max(S, max_scale) < 16777216.0,
               "resized long side out of range");
  if (spatial_idx < 0)
    CSTS_REQUIRE(min_scale >= S && max_scale >= min_scale && max_scale <= 16384,
                 "train mode needs crop_size <= min_scale <= max_scale <= 16384");
  return 0;
}

inline SpatialRule make_rule(int T, int L, int H, int W, int S, int min_scale, int max_scale, int spatial_idx, int random_flip,
                      int inv_uniform) {
  return SpatialRule{T, L, H, W, S, min_scale, max_scale, spatial_idx, random_flip ? 1 : 0, inv_uniform ? 1 : 0};
}

// max(H, W) / min(H, W) * max(S, max_scale) < 2^24: the resized long side stays exact in fp32 (the range spatial_check accepts)
__host__ __device__ __forceinline__ bool spatial_hw_ok(int64_t H, int64_t W, int S, int max_scale) {
  if (H < 1 || W < 1 || H > 16777216 || W > 16777216) return false;
  const double lo = (double)(H < W ? H : W), hi = (double)(H < W ? W : H);
  return hi / lo * (double)(S > max_scale ? S : max_scale) < 16777216.0;
}

// dynamic LDS of a sample launch for source rows of up to W pixels
__host__ __device__ inline int sample_lds_bytes(int W, int* rowcap) {
  *rowcap = (3 * W + 30 + 15) / 16 * 16;
  return SAMPLE_ROWS * 2 * *rowcap;
}

}  // namespace
