// On-device spatial sampling of the training / evaluation clips: the reference's
// slowfast/datasets/utils.py::spatial_sampling(..., gaze_loc=label) (ego4d_avgaze_forecast.py:302-311), i.e.
//   train (spatial_idx -1): random_short_side_scale_jitter -> random_crop_gaze -> horizontal_flip_gaze
//                           (transform.py:43-97, 155-197, 235-262)
//   test  (spatial_idx 0/1/2): short side resized to the crop size -> uniform_crop_gaze (transform.py:327-387)
// include/csts_hip.h states the rule; spatial_rule() below is its one implementation, evaluated on the device by
// spatial_params (one lane per clip, variates from Philox4x32-10 under a key in device memory) and on the host by
// csts_spatial_rule_host (explicit variates).  All rule arithmetic is fp64 without contraction (the Makefile's
// -ffp-contract=off), so sizes and offsets equal numpy's integer for integer.
//
// spatial_sample: one fused pass uint8 (B, T, H, W, 3) -> fp32 (B, 3, T, S, S) = bilinear resize (F.interpolate,
// align_corners=False, no antialias) + crop + flip + (x/255 - mean)/std.  A wave owns one output row: it stages the span of
// the two source rows that row reads in LDS with 16-byte loads, then each lane forms 4 consecutive pixels of every channel
// plane and stores them as one float4 per plane (the output writes are the dominant traffic).
//
// clip_sample: the same pass with an index table in front of it.  The clips are windows of ONE resident video (N, H, W, 3):
// frame t of clip b is video[clamp(frames_idx[b][t], 0, N - 1)], read on the device, so overlapping windows are sampled straight
// out of the video without first being gathered into a (B, T, H, W, 3) tensor of their own.
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

__global__ __launch_bounds__(64) void spatial_params_kernel(const uint64_t* __restrict__ key, const double* __restrict__ labels,
                                                            SpatialRule a, int B, int* __restrict__ params,
                                                            double* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double u[4] = {0.0, 0.0, 0.0, 0.0};
  if (a.spatial_idx < 0) {
    const uint64_t k = *key;
    spatial_uniforms((uint32_t)k, (uint32_t)(k >> 32), (uint64_t)b, u);
  }
  double g[SPATIAL_MAX_T];
  const int64_t off = (int64_t)b * a.T * a.L;
  spatial_rule(labels + off, a, u, params + 5 * b, out + off, g);
}

// grid (ceil(S / 4), T, B), 256 threads; dynamic LDS: 4 waves x 2 source rows x rowcap bytes.
// INDEXED: src is a video of nsrc frames and frames_idx [B][T] names the frame of each (b, t); otherwise frame (b, t) is b * T + t.
template <bool INDEXED>
__global__ __launch_bounds__(256) void spatial_sample_kernel(const uint8_t* __restrict__ src, const int* __restrict__ frames_idx,
                                                             int64_t nsrc, const int* __restrict__ params, float* __restrict__ out,
                                                             int T, int H, int W, int S, int64_t src_bytes, int rowcap, float3 mean,
                                                             float3 inv_std) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * SAMPLE_ROWS + wv;                 // output row of this wave
  const int t = blockIdx.y, b = blockIdx.z;
  const int nh = params[5 * b], nw = params[5 * b + 1], y0 = params[5 * b + 2], x0 = params[5 * b + 3], flip = params[5 * b + 4];
  const int64_t plane = (int64_t)S * S;
  float* o0 = out + ((int64_t)b * 3 * T + t) * plane + (int64_t)i * S;      // channel c at o0 + c * T * plane
  const int64_t cstride = (int64_t)T * plane;
  const bool row_ok = i < S;
  // parameters outside the rule's range (injected by a caller): the clip's output is NaN, nothing is read
  if (nh < S || nw < S || y0 < 0 || x0 < 0 || y0 > nh - S || x0 > nw - S) {
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
  // the source frame: a frame of H * W * 3 bytes starts at any byte, so the 16-byte chunks below are laid out from the byte
  // offset in src (16-byte aligned itself), never from the offset inside the frame
  int64_t frame = (int64_t)b * T + t;
  if (INDEXED) frame = min(max((int64_t)frames_idx[frame], (int64_t)0), nsrc - 1);     // as temporal_sampling clamps
  int shift[2];
  for (int r = 0; r < 2; ++r) {
    const int64_t row0 = (frame * H + (r ? yb : ya)) * W * 3;
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

int spatial_check(int B, int T, int L, int H, int W, int S, int min_scale, int max_scale, int spatial_idx) {
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

SpatialRule make_rule(int T, int L, int H, int W, int S, int min_scale, int max_scale, int spatial_idx, int random_flip,
                      int inv_uniform) {
  return SpatialRule{T, L, H, W, S, min_scale, max_scale, spatial_idx, random_flip ? 1 : 0, inv_uniform ? 1 : 0};
}

// the one launch behind csts_spatial_sample (frames_idx NULL: nsrc = B * T frames in clip order) and csts_clip_sample
template <bool INDEXED>
int launch_sample(const uint8_t* src, const int* frames_idx, int64_t nsrc, const int* params, float* out, int B, int T, int H, int W,
                  int S, const float mean[3], const float std[3], hipStream_t stream) {
  const int rowcap = (3 * W + 30 + 15) / 16 * 16;
  const int lds = SAMPLE_ROWS * 2 * rowcap;
  if (lds > 65536)
    CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&spatial_sample_kernel<INDEXED>), lds), "LDS opt-in");
  const float3 m = make_float3(mean[0], mean[1], mean[2]), is = make_float3(1.f / std[0], 1.f / std[1], 1.f / std[2]);
  const int64_t src_bytes = nsrc * H * W * 3;
  hipLaunchKernelGGL(spatial_sample_kernel<INDEXED>, dim3((unsigned)cdiv(S, SAMPLE_ROWS), T, B), dim3(256), lds, stream, src,
                     frames_idx, nsrc, params, out, T, H, W, S, src_bytes, rowcap, m, is);
  CSTS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int csts_spatial_params(const uint64_t* key, const double* labels, int B, int T, int L, int H, int W, int S, int min_scale,
                                   int max_scale, int spatial_idx, int random_flip, int inv_uniform, int* params,
                                   double* labels_out, hipStream_t stream) {
  if (spatial_check(B, T, L, H, W, S, min_scale, max_scale, spatial_idx)) return -1;
  CSTS_REQUIRE(labels && params && labels_out && (spatial_idx >= 0 || key), "bad args");
  const SpatialRule a = make_rule(T, L, H, W, S, min_scale, max_scale, spatial_idx, random_flip, inv_uniform);
  hipLaunchKernelGGL(spatial_params_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, stream, key, labels, a, B, params, labels_out);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_spatial_sample(const uint8_t* frames_thwc, const int* params, float* out, int B, int T, int H, int W, int S,
                                   const float mean[3], const float std[3], hipStream_t stream) {
  CSTS_REQUIRE(frames_thwc && params && out && mean && std, "bad args");
  CSTS_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && S > 0 && S <= 4096 && W <= 6000 && B <= 65535 && T <= 65535,
               "bad sizes (W <= 6000, S <= 4096)");
  CSTS_REQUIRE(aligned16(frames_thwc) && aligned16(out), "frames and output must be 16-byte aligned");
  return launch_sample<false>(frames_thwc, nullptr, (int64_t)B * T, params, out, B, T, H, W, S, mean, std, stream);
}

extern "C" int csts_clip_sample(const uint8_t* video_nhwc, int64_t N, const int* frames_idx, const int* params, float* out, int B,
                                int T, int H, int W, int S, const float mean[3], const float std[3], hipStream_t stream) {
  CSTS_REQUIRE(video_nhwc && frames_idx && params && out && mean && std, "bad args");
  CSTS_REQUIRE(N >= 1 && B > 0 && T > 0 && T <= SPATIAL_MAX_T && H > 0 && W > 0 && S > 0 && S <= 4096 && W <= 6000 && B <= 65535,
               "bad sizes (N >= 1, T <= 64, W <= 6000, S <= 4096)");
  CSTS_REQUIRE(aligned16(video_nhwc) && aligned16(out), "video and output must be 16-byte aligned");
  return launch_sample<true>(video_nhwc, frames_idx, N, params, out, B, T, H, W, S, mean, std, stream);
}

extern "C" int csts_spatial_rule_host(const double* labels, int B, int T, int L, int H, int W, int S, int min_scale, int max_scale,
                                      int spatial_idx, int random_flip, int inv_uniform, const double* uniforms, int* params,
                                      double* labels_out) {
  if (spatial_check(B, T, L, H, W, S, min_scale, max_scale, spatial_idx)) return -1;
  CSTS_REQUIRE(labels && params && labels_out && (spatial_idx >= 0 || uniforms), "bad args");
  const SpatialRule a = make_rule(T, L, H, W, S, min_scale, max_scale, spatial_idx, random_flip, inv_uniform);
  double g[SPATIAL_MAX_T];
  for (int b = 0; b < B; ++b) {
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t off = (int64_t)b * T * L;
    spatial_rule(labels + off, a, spatial_idx < 0 ? uniforms + 4 * (int64_t)b : zero, params + 5 * (int64_t)b, labels_out + off, g);
  }
  return 0;
}

extern "C" int csts_spatial_uniforms_host(uint32_t key0, uint32_t key1, uint64_t first, int64_t count, double* out) {
  CSTS_REQUIRE(out && count >= 0, "bad args");
  for (int64_t i = 0; i < count; ++i) spatial_uniforms(key0, key1, first + (uint64_t)i, out + 4 * i);
  return 0;
}
