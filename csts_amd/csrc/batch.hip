// One-launch batch assembly from many recordings (csts_amd/datasets.py): a training batch is B clips of B different recordings,
// possibly of B frame sizes, all resident in arenas on the device.  The three kernels read their per-clip tables on the device
// (no host sync, no allocation, no atomics: graph-capturable; rewriting the tables between replays assembles the next batch).
//
//   batch_params : spatial_params (spatial.hip) with H, W of clip b taken from the clip table; clip b draws the variates u[b].
//   batch_sample : the pixel pass of spatial_sample / clip_sample (sample_rows, spatial_shared.h) with clip b read from its own
//                  recording inside one uint8 arena.  A table row whose extent leaves the arena gives a NaN clip and reads nothing.
//   audio_gather : audio_windows (input.hip) with window (b, t) cut from the spectrogram of clip b inside one fp32 arena.
#include "spatial_shared.h"

namespace {

// row b of the clip table {byte offset, N, H, W}: the recording lies inside [0, arena_bytes) and a row of it fits the staged LDS
__device__ __forceinline__ bool clip_row_ok(const int64_t* __restrict__ row, int64_t arena_bytes, int max_W) {
  const int64_t off = row[0], N = row[1], H = row[2], W = row[3];
  if (off < 0 || off > arena_bytes || N < 1 || H < 1 || W < 1 || W > max_W || H > 0x7fffffff || N > 0x7fffffff) return false;
  return N <= (arena_bytes - off) / (H * W * 3);          // H W 3 < 2^46: no overflow; N H W 3 is never formed
}

__global__ __launch_bounds__(64) void batch_params_kernel(const uint64_t* __restrict__ key, const double* __restrict__ labels,
                                                          const int64_t* __restrict__ clips, SpatialRule a, int B,
                                                          int* __restrict__ params, double* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t H = clips[4 * b + 2], W = clips[4 * b + 3];
  const int64_t off = (int64_t)b * a.T * a.L;
  if (!spatial_hw_ok(H, W, a.S, a.max_scale)) {           // a frame size the rule does not take: params no sample pass accepts
    for (int k = 0; k < 5; ++k) params[5 * b + k] = -1;
    for (int k = 0; k < a.T * a.L; ++k) out[off + k] = __builtin_nan("");
    return;
  }
  a.H = (int)H;
  a.W = (int)W;
  double u[4] = {0.0, 0.0, 0.0, 0.0};
  if (a.spatial_idx < 0) {
    const uint64_t k = *key;
    spatial_uniforms((uint32_t)k, (uint32_t)(k >> 32), (uint64_t)b, u);
  }
  double g[SPATIAL_MAX_T];
  spatial_rule(labels + off, a, u, params + 5 * b, out + off, g);
}

// grid (ceil(S / 4), T, B), 256 threads; dynamic LDS sized from max_W (sample_lds_bytes)
__global__ __launch_bounds__(256) void batch_sample_kernel(const uint8_t* __restrict__ arena, int64_t arena_bytes,
                                                           const int64_t* __restrict__ clips, const int* __restrict__ frames_idx,
                                                           const int* __restrict__ params, float* __restrict__ out, int T, int S,
                                                           int max_W, int rowcap, float3 mean, float3 inv_std) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int t = blockIdx.y, b = blockIdx.z;
  const int64_t* row = clips + 4 * b;
  const bool ok = clip_row_ok(row, arena_bytes, max_W);   // uniform over the workgroup (one clip)
  int64_t frame = 0;
  if (ok) frame = min(max((int64_t)frames_idx[(int64_t)b * T + t], (int64_t)0), row[1] - 1);     // as temporal_sampling clamps
  sample_rows(arena, arena_bytes, ok ? row[0] : 0, frame, ok ? (int)row[2] : 1, ok ? (int)row[3] : 1, params + 5 * b, !ok, out, b, t,
              T, S, rowcap, mean, inv_std, lds);
}

// grid (blocks over nbins * width / 4, B * T), 256 threads.  VEC: width % 4 == 0 and out 16-byte aligned, one float4 store per lane
template <bool VEC>
__global__ __launch_bounds__(256) void audio_gather_kernel(const float* __restrict__ arena, const int64_t* __restrict__ specs,
                                                           const int* __restrict__ centers, float* __restrict__ out, int T, int nbins,
                                                           int width) {
  const int bt = blockIdx.y, b = bt / T;
  const int64_t off = specs[3 * b], stride = specs[3 * b + 1], usable = specs[3 * b + 2];
  const int64_t total = (int64_t)nbins * width;
  float* o = out + (int64_t)bt * total;
  const int half = width / 2;
  const bool ok = off >= 0 && usable >= (int64_t)width + 1 && usable <= stride;
  // a row no window fits in: NaN windows, nothing is read
  const int64_t c = ok ? min(max((int64_t)centers[bt], (int64_t)half), usable - 1 - half) : 0;
  const float* s = arena + off + c - half;
  constexpr int V = VEC ? 4 : 1;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (int64_t)gridDim.x * 256 * V) {
    const int bin = (int)(i / width), j = (int)(i - (int64_t)bin * width);
    if (VEC) {
      float4 v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
      if (ok) {
        const float* p = s + (int64_t)bin * stride + j;    // the window starts at any column: four dword loads
        v = make_float4(p[0], p[1], p[2], p[3]);
      }
      *reinterpret_cast<float4*>(o + i) = v;
    } else {
      o[i] = ok ? s[(int64_t)bin * stride + j] : __builtin_nanf("");
    }
  }
}

}  // namespace

extern "C" int csts_batch_params(const uint64_t* key, const double* labels, const int64_t* clips, int B, int T, int L, int S,
                                 int min_scale, int max_scale, int spatial_idx, int random_flip, int inv_uniform, int* params,
                                 double* labels_out, hipStream_t stream) {
  if (spatial_check(B, T, L, 1, 1, S, min_scale, max_scale, spatial_idx)) return -1;
  CSTS_REQUIRE(labels && clips && params && labels_out && (spatial_idx >= 0 || key), "bad args");
  const SpatialRule a = make_rule(T, L, 1, 1, S, min_scale, max_scale, spatial_idx, random_flip, inv_uniform);
  hipLaunchKernelGGL(batch_params_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, stream, key, labels, clips, a, B, params,
                     labels_out);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_batch_sample(const uint8_t* arena_u8, int64_t arena_bytes, const int64_t* clips, const int* frames_idx,
                                 const int* params, float* out, int B, int T, int S, int max_W, const float mean[3],
                                 const float std[3], hipStream_t stream) {
  CSTS_REQUIRE(arena_u8 && clips && frames_idx && params && out && mean && std, "bad args");
  CSTS_REQUIRE(arena_bytes >= 3 && B > 0 && B <= 65535 && T > 0 && T <= SPATIAL_MAX_T && S > 0 && S <= 4096 && max_W > 0 &&
                   max_W <= 6000, "bad sizes (T <= 64, max_W <= 6000, S <= 4096)");
  CSTS_REQUIRE(aligned16(arena_u8) && aligned16(out), "arena and output must be 16-byte aligned");
  int rowcap;
  const int lds = sample_lds_bytes(max_W, &rowcap);
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&batch_sample_kernel), lds), "LDS opt-in");
  const float3 m = make_float3(mean[0], mean[1], mean[2]), is = make_float3(1.f / std[0], 1.f / std[1], 1.f / std[2]);
  hipLaunchKernelGGL(batch_sample_kernel, dim3((unsigned)cdiv(S, SAMPLE_ROWS), T, B), dim3(256), lds, stream, arena_u8, arena_bytes,
                     clips, frames_idx, params, out, T, S, max_W, rowcap, m, is);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_audio_gather(const float* spec_arena, const int64_t* specs, const int* centers, float* out, int B, int T,
                                 int nbins, int width, hipStream_t stream) {
  CSTS_REQUIRE(spec_arena && specs && centers && out && B > 0 && T > 0 && nbins > 0 && width > 0 && (int64_t)B * T <= 65535,
               "bad args (B * T <= 65535)");
  CSTS_REQUIRE((width & 1) == 0, "width must be even: a window is the columns [c - width/2, c + width/2)");
  const bool vec = (width & 3) == 0 && aligned16(out);
  const int64_t per = vec ? 1024 : 256;
  const dim3 grid((unsigned)std::min<int64_t>(cdiv((int64_t)nbins * width, per), 1024), B * T);
  if (vec)
    hipLaunchKernelGGL(audio_gather_kernel<true>, grid, dim3(256), 0, stream, spec_arena, specs, centers, out, T, nbins, width);
  else
    hipLaunchKernelGGL(audio_gather_kernel<false>, grid, dim3(256), 0, stream, spec_arena, specs, centers, out, T, nbins, width);
  CSTS_LAUNCH_CHECK();
  return 0;
}
