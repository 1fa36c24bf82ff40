// On-device spatial sampling of the training / evaluation clips: the reference's
// slowfast/datasets/utils.py::spatial_sampling(..., gaze_loc=label) (ego4d_avgaze_forecast.py:302-311), i.e.
//   train (spatial_idx -1): random_short_side_scale_jitter -> random_crop_gaze -> horizontal_flip_gaze
//                           (transform.py:43-97, 155-197, 235-262)
//   test  (spatial_idx 0/1/2): short side resized to the crop size -> uniform_crop_gaze (transform.py:327-387)
// include/csts_hip.h states the rule; spatial_rule() (spatial_shared.h, shared with batch.hip) is its one implementation, evaluated on the device by
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
#include "spatial_shared.h"

namespace {

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
  const int t = blockIdx.y, b = blockIdx.z;
  int64_t frame = (int64_t)b * T + t;
  if (INDEXED) frame = min(max((int64_t)frames_idx[frame], (int64_t)0), nsrc - 1);     // as temporal_sampling clamps
  sample_rows(src, src_bytes, 0, frame, H, W, params + 5 * b, false, out, b, t, T, S, rowcap, mean, inv_std, lds);
}

// the one launch behind csts_spatial_sample (frames_idx NULL: nsrc = B * T frames in clip order) and csts_clip_sample
template <bool INDEXED>
int launch_sample(const uint8_t* src, const int* frames_idx, int64_t nsrc, const int* params, float* out, int B, int T, int H, int W,
                  int S, const float mean[3], const float std[3], hipStream_t stream) {
  int rowcap;
  const int lds = sample_lds_bytes(W, &rowcap);
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
