// Live-stream input (csts_amd/stream.py): frames and audio arrive in pieces of any size and the recording never ends, so what the
// windows read lives in two device rings whose size does not depend on the length of the stream.
//   stream_stft          : columns [f0, f1) of the log-power STFT of the endless signal, from the buffer that holds the samples they
//                          need, into a spectrogram ring at column f mod ring_cols.  The column body is stft_logpower_column
//                          (stft_shared.h), the one csts_stft_logpower runs: a column has the bits it has offline.
//   stream_audio_windows : the T windows of 256 columns around global centre columns, read out of the ring across its wrap.
//   stream_ingest(_yuv)  : the frames of one pushed chunk some window will read, sampled ONCE into a ring of normalised crops by
//                          sample_rows / sample_rows_yuv (the pixel pass of csts_clip_sample) under one test-mode parameter row.
//   stream_gather        : (B, 3, T, S, S) clips out of the crop ring by a slot table.
//   live_track_add       : the maps of newly run windows folded into a ring of per-frame sums (frame t in slot t mod Rt).
//   live_track_rows      : the rows of a gaze track for the frames just pushed, out of that ring: mean, neighbours, hold or blend,
//                          decode -- the device functions of csts_gaze_track / csts_gaze_track_fill (track_shared.h).
//   group_stft, group_audio_windows, group_ingest(_yuv) : stream_stft, stream_audio_windows and stream_ingest(_yuv) for the
//                          streams of a GazeStreamGroup, which share one arena of rings: one launch takes what several streams
//                          pushed, from a job table; the column, the window and the crop are computed by the same device functions.
//   group_live_add, group_live_rows : live_track_add and live_track_rows for the slots of a GazeLiveGroup, whose track rings share
//                          one arena: one launch folds the windows of all slots, one answers the frames of all slots, from a
//                          (stream, target) and a (stream, frame) table; the slot and the row are live_add_slot and live_row, the
//                          device functions the single-stream kernels run.
// Every table is DEVICE memory read when the kernel runs; no atomics, no allocation, no synchronisation.
#include <vector>

#include "stft_shared.h"
#include "yuv_shared.h"
#include "track_shared.h"

namespace {

// grid (f1 - f0), 256 threads; dynamic LDS stft_lds_floats.  buf holds the samples [s_base, s_base + m); samples below 0, and with
// n_total >= 0 those at or past n_total, are zero.  A sample the buffer does not hold reads nothing (the host refuses the launch).
__global__ __launch_bounds__(256) void stream_stft_kernel(const float* __restrict__ buf, int64_t s_base, int64_t m, int64_t n_total,
                                                          int64_t f0, float* __restrict__ ring, int ring_cols, int n_fft, int hop,
                                                          int win, float eps) {
  extern __shared__ float sm[];
  const int64_t f = f0 + blockIdx.x;
  const int64_t s_end = s_base + m;
  stft_logpower_column(sm, f, n_fft, hop, win, eps,
                       [=](int64_t s) { return s >= 0 && (n_total < 0 || s < n_total) && s >= s_base && s < s_end; },
                       [=](int64_t s) { return buf[s - s_base]; }, ring + (int)(f % ring_cols), ring_cols);
}

// grid (blocks over nbins * width / V, B * T), 256 threads.  out[bt][bin][j] = ring[bin][(centers[bt] - width / 2 + j) mod ring_cols];
// a window not wholly inside the live span [max(newest - ring_cols + 1, 0), newest] is NaN and reads nothing.
// VEC: width % 4 == 0 and out 16-byte aligned, one float4 store per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void stream_audio_windows_kernel(const float* __restrict__ ring, int ring_cols, int64_t newest,
                                                                   const int64_t* __restrict__ centers, float* __restrict__ out,
                                                                   int nbins, int width) {
  const int bt = blockIdx.y;
  const int64_t lo = centers[bt] - width / 2, hi = lo + width - 1;
  const int64_t oldest = newest - ring_cols + 1 > 0 ? newest - ring_cols + 1 : 0;
  const bool ok = lo >= oldest && hi <= newest;            // uniform over the workgroup (one window)
  const int start = ok ? (int)(lo % ring_cols) : 0;
  const int64_t total = (int64_t)nbins * width;
  float* o = out + (int64_t)bt * total;
  constexpr int V = VEC ? 4 : 1;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (int64_t)gridDim.x * 256 * V) {
    const int bin = (int)(i / width), j = (int)(i - (int64_t)bin * width);
    const float* row = ring + (int64_t)bin * ring_cols;
    float v[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      int c = start + j + q;                               // < 2 ring_cols: width <= ring_cols
      if (c >= ring_cols) c -= ring_cols;
      v[q] = ok ? row[c] : __builtin_nanf("");
    }
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(o + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      o[i] = v[0];
    }
  }
}

// one row of the (frame in chunk, slot) table: inside the chunk and the ring, or the workgroup writes nothing
__device__ __forceinline__ bool ingest_pair_ok(const int* __restrict__ pairs, int p, int K, int R, int* frame, int* slot) {
  *frame = pairs[2 * p];
  *slot = pairs[2 * p + 1];
  return *frame >= 0 && *frame < K && *slot >= 0 && *slot < R;
}

// grid (ceil(S / 4), pairs), 256 threads; dynamic LDS sample_lds_bytes(W).  The ring is (R, 3, S, S): slot r is "clip" r of one frame
__global__ __launch_bounds__(256) void stream_ingest_kernel(const uint8_t* __restrict__ chunk, int K, int H, int W,
                                                            const int* __restrict__ pairs, const int* __restrict__ params,
                                                            float* __restrict__ ring, int R, int S, int64_t chunk_bytes, int rowcap,
                                                            float3 mean, float3 inv_std) {
  extern __shared__ __align__(16) uint8_t lds[];
  int frame, slot;
  if (!ingest_pair_ok(pairs, blockIdx.y, K, R, &frame, &slot)) return;      // uniform over the workgroup (one pair)
  sample_rows(chunk, chunk_bytes, 0, frame, H, W, params, false, ring, slot, 0, 1, S, rowcap, mean, inv_std, lds);
}

// the same for a chunk of 4:2:0 frames, the H x W pictures of the surfaces sf; dynamic LDS sample_yuv_lds_bytes(W)
__global__ __launch_bounds__(256) void stream_ingest_yuv_kernel(const uint8_t* __restrict__ chunk, int K, int H, int W, YuvSurf sf,
                                                                const int* __restrict__ pairs, const int* __restrict__ params,
                                                                float* __restrict__ ring, int R, int S, int64_t chunk_bytes, int lcap,
                                                                int ccap, int layout, YuvCoef k, float3 mean, float3 inv_std) {
  extern __shared__ __align__(16) uint8_t lds[];
  int frame, slot;
  if (!ingest_pair_ok(pairs, blockIdx.y, K, R, &frame, &slot)) return;
  sample_rows_yuv(chunk, chunk_bytes, 0, frame, H, W, sf, params, false, ring, slot, 0, 1, S, lcap, ccap, layout, k, mean, inv_std, lds);
}

// grid (blocks over S * S / V, 3 * T, B), 256 threads.  out[b][c][t] = ring[slots[b][t]][c]; a slot outside [0, R) gives NaN.
// VEC: S * S % 4 == 0 and both 16-byte aligned, one float4 per lane each way.
template <bool VEC>
__global__ __launch_bounds__(256) void stream_gather_kernel(const float* __restrict__ ring, int R, const int* __restrict__ slots,
                                                            float* __restrict__ out, int T, int64_t plane) {
  const int c = blockIdx.y / T, t = blockIdx.y - c * T, b = blockIdx.z;
  const int slot = slots[(int64_t)b * T + t];
  const bool ok = slot >= 0 && slot < R;                   // uniform over the workgroup
  const float* src = ring + ((int64_t)(ok ? slot : 0) * 3 + c) * plane;
  float* dst = out + (((int64_t)b * 3 + c) * T + t) * plane;
  constexpr int V = VEC ? 4 : 1;
  const float nan = __builtin_nanf("");
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < plane; i += (int64_t)gridDim.x * 256 * V) {
    if constexpr (VEC)
      *reinterpret_cast<float4*>(dst + i) = ok ? *reinterpret_cast<const float4*>(src + i) : make_float4(nan, nan, nan, nan);
    else
      dst[i] = ok ? src[i] : nan;
  }
}

// ---- live track ring (GazeStream(live=...)): frame t lives in slot t mod Rt of sum (Rt, hw) / count (Rt) / tag (Rt), the tag
// being the frame number the slot holds (-1: empty).  A slot is written by ONE workgroup of ONE launch at a time and read by a
// later launch on the same stream: plain loads and stores, no atomics.  Inside that workgroup every lane reads the slot's tag and
// count before a workgroup barrier and lane 0 writes them after it; a lane reads and writes only its own cells of the sum.

// One track slot (`slot` of a ring of Rt; dst its sum, cnt_at and tag_at its count and tag) takes the rows of maps [P][hw] that
// target it.  row_target(p) is the frame row p predicts, or a negative number when the row is not for this ring; it must depend
// on p and device tables alone, so that every read of it is uniform over the workgroup.  The rows are walked in ascending p and
// those whose target t >= 0 has t mod Rt == slot are taken:  tag != t -> the slot restarts (sum = 0 + row, count = 1, tag = t);
// tag == t -> sum += row, count += 1.  The walk is done twice: once on the tags alone, which finds the slot's last restart
// (`start`, -1: none: the sum in the ring is carried on), its final tag and count; then per 4-cell chunk over the rows from there
// on, so that a cell is read once per row that counts and written once.  The additions of one cell are ((0 + row_0) + row_1) +
// ..., in window order across calls and in ascending p inside one: the order of csts_gaze_track.  A slot no row names is not
// touched.  The one statement of the rule: live_track_add_kernel and group_live_add_kernel both run it, so a track slot has the
// bits it has in a single stream.
template <bool VEC, class RowTarget>
__device__ __forceinline__ void live_add_slot(const float* __restrict__ maps, int P, int hw, float* __restrict__ dst,
                                              int* __restrict__ cnt_at, int64_t* __restrict__ tag_at, int slot, int Rt,
                                              RowTarget row_target) {
  const int tid = threadIdx.x;
  int64_t cur = *tag_at;
  int cnt = *cnt_at, start = -1, hits = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t t = row_target(p);
    if (t < 0 || (int)(t % Rt) != slot) continue;
    ++hits;
    if (t != cur) { cur = t; cnt = 1; start = p; } else { ++cnt; }
  }
  if (hits == 0) return;                                     // uniform over the workgroup: it depends on the tables alone
  // Every lane has read the slot's tag and count by here; lane 0 replaces them at the end.  Without this barrier a wave that
  // started late could read the NEW tag of a restarted slot, take the restart for a carry-on and add to the old frame's sum.
  __syncthreads();
  const int first = start < 0 ? 0 : start;
  constexpr int V = VEC ? 4 : 1;
  for (int at = tid * V; at < hw; at += 256 * V) {
    float acc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = 0.f;
    if (start < 0) {
      if constexpr (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(dst + at);
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = v[q];
      } else {
        acc[0] = dst[at];
      }
    }
    for (int p = first; p < P; ++p) {
      if (row_target(p) != cur) continue;                    // from `start` on, the slot's rows all carry its final tag (>= 0)
      const float* row = maps + (int64_t)p * hw + at;
      if constexpr (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row);
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] += v[q];
      } else {
        acc[0] += row[0];
      }
    }
    if constexpr (VEC) {
      f32x4 o;
#pragma unroll
      for (int q = 0; q < V; ++q) o[q] = acc[q];
      *reinterpret_cast<f32x4*>(dst + at) = o;
    } else {
      dst[at] = acc[0];
    }
  }
  if (tid == 0) { *cnt_at = cnt; *tag_at = cur; }
}

// grid (Rt), 256 threads.  Workgroup s is slot s of the ring and takes the rows of target[0 .. P) by live_add_slot.
template <bool VEC>
__global__ __launch_bounds__(256) void live_track_add_kernel(const float* __restrict__ maps, const int64_t* __restrict__ target, int P,
                                                             int hw, float* __restrict__ sum, int* __restrict__ count,
                                                             int64_t* __restrict__ tag, int Rt) {
  const int slot = blockIdx.x;
  live_add_slot<VEC>(maps, P, hw, sum + (int64_t)slot * hw, count + slot, tag + slot, slot, Rt, [=](int p) { return target[p]; });
}

// grid (Rt, streams), 256 threads: the track rings of a GazeLiveGroup lie in one arena, sum (streams, Rt, hw), count and tag
// (streams, Rt).  Workgroup (s, i) is live_track_add_kernel's workgroup s on the ring of stream i, restricted to the rows with
// stream_of[p] == i; a row whose stream lies outside [0, streams) belongs to no workgroup.  Both tables are read by blockIdx and
// p alone: uniform loads.
template <bool VEC>
__global__ __launch_bounds__(256) void group_live_add_kernel(const float* __restrict__ maps, const int64_t* __restrict__ target,
                                                             const int* __restrict__ stream_of, int P, int hw,
                                                             float* __restrict__ sum, int* __restrict__ count,
                                                             int64_t* __restrict__ tag, int Rt) {
  const int slot = blockIdx.x, i = blockIdx.y;
  const int64_t at = (int64_t)i * Rt + slot;
  live_add_slot<VEC>(maps, P, hw, sum + at * hw, count + at, tag + at, slot, Rt,
                     [=](int p) { return stream_of[p] == i ? target[p] : (int64_t)-1; });
}

// how many maps frame t holds in the ring: its slot's count when the slot's tag is t, else 0 (never written, or recycled)
__device__ __forceinline__ int live_count_of(const int* __restrict__ count, const int64_t* __restrict__ tag, int Rt, int64_t t) {
  if (t < 0) return 0;
  const int s = (int)(t % Rt);
  return tag[s] == t ? count[s] : 0;
}

// frame t's mean map out of the ring, in registers: sum * (1 / count), csts_gaze_track's mean
template <int NCH, bool VEC>
__device__ __forceinline__ void live_mean(float (&m)[NCH * 4], const float* __restrict__ sum, const int* __restrict__ count, int Rt,
                                          int64_t t, int hw, int tid) {
  const int s = (int)(t % Rt);
  load_map<NCH, VEC>(m, sum + (int64_t)s * hw, hw, tid);
  const float inv = 1.f / (float)count[s];
#pragma unroll
  for (int k = 0; k < NCH * 4; ++k) m[k] *= inv;
}

// Workgroup blockIdx.x answers frame n of the ring (sum, count, tag) by the rule of csts_gaze_track_fill on a track of
// n + max_gap + 1 frames whose count is live_count_of: a, b as gaze_fill_kernel finds them (all uniform over the workgroup), the
// map by live_mean / blend_maps, the outputs by track_tail, into row blockIdx.x.  n < 0 finds nothing: the unpredicted row.
template <int NCH, bool VEC>
__device__ __forceinline__ void live_row(const float* __restrict__ sum, const int* __restrict__ count, const int64_t* __restrict__ tag,
                                         int Rt, int64_t n, int H, int W, int mode, int max_gap, float* __restrict__ heatmaps,
                                         float* __restrict__ rescaled, float* __restrict__ points, float* __restrict__ peak,
                                         int* __restrict__ out_count, int* __restrict__ neighbours) {
  const int tid = threadIdx.x;
  const int hw = H * W;
  const int own = live_count_of(count, tag, Rt, n);
  int64_t a = -1, b = -1;
  if (own > 0) {
    a = b = n;
  } else {
    const int64_t lo = n - (max_gap - 1) > 0 ? n - (max_gap - 1) : 0;
    for (int64_t j = n - 1; j >= lo; --j)
      if (live_count_of(count, tag, Rt, j) > 0) { a = j; break; }
    if (a >= 0) {
      const int64_t hi = a + max_gap;                        // b - a <= max_gap; the track ends at n + max_gap > hi
      for (int64_t j = n + 1; j <= hi; ++j)
        if (live_count_of(count, tag, Rt, j) > 0) { b = j; break; }
    }
    if (b < 0) a = -1;
  }
  float m[NCH * 4];
  if (a < 0) {
#pragma unroll
    for (int k = 0; k < NCH * 4; ++k) m[k] = 0.f;
  } else {
    live_mean<NCH, VEC>(m, sum, count, Rt, a, hw, tid);
    if (mode == 1 && b != a) {
      float hb[NCH * 4];
      live_mean<NCH, VEC>(hb, sum, count, Rt, b, hw, tid);
      blend_maps<NCH>(m, hb, a, b, n);
    }
  }
  track_tail<NCH, VEC>(m, a >= 0, H, W, heatmaps, rescaled, points, peak);
  if (tid == 0) {
    if (out_count) out_count[blockIdx.x] = own;
    if (neighbours) { neighbours[2 * (int64_t)blockIdx.x] = (int)a; neighbours[2 * (int64_t)blockIdx.x + 1] = (int)b; }
  }
}

// grid (K), 256 threads: workgroup k answers frame f0 + k
template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void live_track_rows_kernel(const float* __restrict__ sum, const int* __restrict__ count,
                                                              const int64_t* __restrict__ tag, int Rt, int64_t f0, int H, int W,
                                                              int mode, int max_gap, float* __restrict__ heatmaps,
                                                              float* __restrict__ rescaled, float* __restrict__ points,
                                                              float* __restrict__ peak, int* __restrict__ out_count,
                                                              int* __restrict__ neighbours) {
  live_row<NCH, VEC>(sum, count, tag, Rt, f0 + blockIdx.x, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count,
                     neighbours);
}

// grid (K), 256 threads: workgroup k answers frame frame_of[k] of the ring of stream stream_of[k] in the arena of
// group_live_add_kernel, by live_row.  Both table reads depend on blockIdx alone: uniform.  A stream outside [0, streams), or
// a negative frame, gives the unpredicted row and reads no ring.
template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void group_live_rows_kernel(const float* __restrict__ sum, const int* __restrict__ count,
                                                              const int64_t* __restrict__ tag, int streams, int Rt,
                                                              const int* __restrict__ stream_of, const int64_t* __restrict__ frame_of,
                                                              int H, int W, int mode, int max_gap, float* __restrict__ heatmaps,
                                                              float* __restrict__ rescaled, float* __restrict__ points,
                                                              float* __restrict__ peak, int* __restrict__ out_count,
                                                              int* __restrict__ neighbours) {
  const int i = stream_of[blockIdx.x];
  const bool known = i >= 0 && i < streams;
  const int64_t ring = (int64_t)(known ? i : 0) * Rt;
  live_row<NCH, VEC>(sum + ring * (H * W), count + ring, tag + ring, Rt, known ? frame_of[blockIdx.x] : (int64_t)-1, H, W, mode,
                     max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
}

template <int NCH>
void launch_live_rows(bool vec, unsigned K, hipStream_t stream, const float* sum, const int* count, const int64_t* tag, int Rt,
                      int64_t f0, int H, int W, int mode, int max_gap, float* heatmaps, float* rescaled, float* points, float* peak,
                      int* out_count, int* neighbours) {
  if (vec) hipLaunchKernelGGL((live_track_rows_kernel<NCH, true>), dim3(K), dim3(256), 0, stream, sum, count, tag, Rt, f0, H, W, mode,
                              max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  else hipLaunchKernelGGL((live_track_rows_kernel<NCH, false>), dim3(K), dim3(256), 0, stream, sum, count, tag, Rt, f0, H, W, mode,
                          max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
}

template <int NCH>
void launch_group_live_rows(bool vec, unsigned K, hipStream_t stream, const float* sum, const int* count, const int64_t* tag,
                            int streams, int Rt, const int* stream_of, const int64_t* frame_of, int H, int W, int mode, int max_gap,
                            float* heatmaps, float* rescaled, float* points, float* peak, int* out_count, int* neighbours) {
  if (vec) hipLaunchKernelGGL((group_live_rows_kernel<NCH, true>), dim3(K), dim3(256), 0, stream, sum, count, tag, streams, Rt,
                              stream_of, frame_of, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  else hipLaunchKernelGGL((group_live_rows_kernel<NCH, false>), dim3(K), dim3(256), 0, stream, sum, count, tag, streams, Rt,
                          stream_of, frame_of, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
}

int ingest_check(const void* chunk, const void* pairs, const void* params, const void* ring, const float* mean, const float* std,
                 int K, int H, int W, int npairs, int R, int S) {
  CSTS_REQUIRE(chunk && pairs && params && ring && mean && std, "bad args");
  CSTS_REQUIRE(K > 0 && H > 0 && W > 0 && W <= 6000 && npairs > 0 && npairs <= 65535 && R > 0 && S > 0 && S <= 4096 &&
                   (int64_t)R * 3 * S * S < ((int64_t)1 << 40), "bad sizes (W <= 6000, S <= 4096, pairs <= 65535)");
  CSTS_REQUIRE(aligned16(chunk) && aligned16(ring), "chunk and ring must be 16-byte aligned");
  return 0;
}

// ---- stream group (GazeStreamGroup): N streams share one arena of crop rings (streams * R, 3, S, S) and one of spectrum rings
// (streams, nbins, ring_cols); what several streams pushed in one tick goes in with ONE launch per stage, from a job table in
// device memory.  A workgroup finds its job from blockIdx alone, so every table read is a uniform (scalar) load, and then runs
// the device function the single-stream kernel runs: a column, a crop, a window has the bits it has there.

constexpr int GROUP_STFT_JOB = 8;      // int64 per row: sample buffer, s_base, m, n_total, f0, f1, stream, first workgroup
constexpr int GROUP_INGEST_JOB = 6;    // int64 per row: chunk, chunk bytes, K, H, W, LDS row capacity

// grid (total columns), 256 threads; dynamic LDS stft_lds_floats.  The rows are ordered by their first workgroup (a running sum
// of f1 - f0, which the host checks): the job of workgroup g is the LAST row whose first workgroup is <= g, which skips the rows
// without columns.  A row whose stream lies outside [0, streams) writes nothing.
__global__ __launch_bounds__(256) void group_stft_kernel(const int64_t* __restrict__ jobs, int njobs, float* __restrict__ rings,
                                                         int streams, int nbins, int ring_cols, int n_fft, int hop, int win,
                                                         float eps) {
  extern __shared__ float sm[];
  const int64_t g = blockIdx.x;
  int lo = 0, hi = njobs - 1;                                 // uniform over the workgroup: blockIdx and the table alone
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[(int64_t)mid * GROUP_STFT_JOB + 7] <= g) lo = mid; else hi = mid - 1;
  }
  const int64_t* job = jobs + (int64_t)lo * GROUP_STFT_JOB;
  const float* buf = reinterpret_cast<const float*>(job[0]);
  const int64_t s_base = job[1], s_end = s_base + job[2], n_total = job[3], f0 = job[4], f1 = job[5], slot = job[6];
  const int64_t f = f0 + (g - job[7]);
  if (slot < 0 || slot >= streams || f < f0 || f >= f1) return;
  float* ring = rings + slot * (int64_t)nbins * ring_cols;
  stft_logpower_column(sm, f, n_fft, hop, win, eps,
                       [=](int64_t s) { return s >= 0 && (n_total < 0 || s < n_total) && s >= s_base && s < s_end; },
                       [=](int64_t s) { return buf[s - s_base]; }, ring + (int)(f % ring_cols), ring_cols);
}

// grid (blocks over nbins * width / V, B * T), 256 threads: stream_audio_windows_kernel with the ring and its newest column
// looked up per batch row: row b reads ring stream_of[b] under newest[stream_of[b]]; a stream outside [0, streams) is NaN.
template <bool VEC>
__global__ __launch_bounds__(256) void group_audio_windows_kernel(const float* __restrict__ rings, int streams, int ring_cols,
                                                                  const int* __restrict__ stream_of,
                                                                  const int64_t* __restrict__ newest_of,
                                                                  const int64_t* __restrict__ centers, float* __restrict__ out, int T,
                                                                  int nbins, int width) {
  const int bt = blockIdx.y;
  const int s = stream_of[bt / T];
  const bool known = s >= 0 && s < streams;                // uniform over the workgroup (one window)
  const int64_t newest = known ? newest_of[s] : -1;
  const int64_t lo = centers[bt] - width / 2, hi = lo + width - 1;
  const int64_t oldest = newest - ring_cols + 1 > 0 ? newest - ring_cols + 1 : 0;
  const bool ok = known && lo >= oldest && hi <= newest;
  const int start = ok ? (int)(lo % ring_cols) : 0;
  const int64_t total = (int64_t)nbins * width;
  const float* ring = rings + (int64_t)(ok ? s : 0) * nbins * ring_cols;
  float* o = out + (int64_t)bt * total;
  constexpr int V = VEC ? 4 : 1;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V; i < total; i += (int64_t)gridDim.x * 256 * V) {
    const int bin = (int)(i / width), j = (int)(i - (int64_t)bin * width);
    const float* row = ring + (int64_t)bin * ring_cols;
    float v[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      int c = start + j + q;                               // < 2 ring_cols: width <= ring_cols
      if (c >= ring_cols) c -= ring_cols;
      v[q] = ok ? row[c] : __builtin_nanf("");
    }
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(o + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      o[i] = v[0];
    }
  }
}

// one row of the (job, frame in chunk, arena slot) table and its job: inside the table, the chunk and the arena, or the workgroup
// writes nothing.  All of it is uniform over the workgroup (one pair).
__device__ __forceinline__ const int64_t* group_pair_job(const int64_t* __restrict__ jobs, int njobs, const int* __restrict__ pairs,
                                                         int p, int arena_slots, int* j, int* frame, int* slot) {
  *j = pairs[3 * p];
  *frame = pairs[3 * p + 1];
  *slot = pairs[3 * p + 2];
  if (*j < 0 || *j >= njobs || *slot < 0 || *slot >= arena_slots) return nullptr;
  const int64_t* job = jobs + (int64_t)*j * GROUP_INGEST_JOB;
  return *frame >= 0 && *frame < job[2] ? job : nullptr;
}

// grid (ceil(S / 4), pairs), 256 threads; dynamic LDS lds_bytes = sample_lds_bytes of the widest job.  A job whose row capacity is
// not the one its W asks for, or does not fit the launch's LDS, writes nothing.
__global__ __launch_bounds__(256) void group_ingest_kernel(const int64_t* __restrict__ jobs, int njobs, const int* __restrict__ params,
                                                           const int* __restrict__ pairs, float* __restrict__ arena, int arena_slots,
                                                           int S, int lds_bytes, float3 mean, float3 inv_std) {
  extern __shared__ __align__(16) uint8_t lds[];
  int j, frame, slot;
  const int64_t* job = group_pair_job(jobs, njobs, pairs, blockIdx.y, arena_slots, &j, &frame, &slot);
  if (!job) return;
  const int H = (int)job[3], W = (int)job[4];
  int rowcap;
  if (sample_lds_bytes(W, &rowcap) > lds_bytes || job[5] != rowcap) return;
  sample_rows(reinterpret_cast<const uint8_t*>(job[0]), job[1], 0, frame, H, W, params + 5 * j, false, arena, slot, 0, 1, S, rowcap,
              mean, inv_std, lds);
}

// the same for chunks of 4:2:0 frames; the job's row capacity is the luma one, lcap of sample_yuv_lds_bytes
__global__ __launch_bounds__(256) void group_ingest_yuv_kernel(const int64_t* __restrict__ jobs, int njobs,
                                                               const int* __restrict__ params, const int* __restrict__ pairs,
                                                               float* __restrict__ arena, int arena_slots, int S, int lds_bytes,
                                                               int layout, YuvCoef k, float3 mean, float3 inv_std) {
  extern __shared__ __align__(16) uint8_t lds[];
  int j, frame, slot;
  const int64_t* job = group_pair_job(jobs, njobs, pairs, blockIdx.y, arena_slots, &j, &frame, &slot);
  if (!job) return;
  const int H = (int)job[3], W = (int)job[4];
  int lcap, ccap;
  if (sample_yuv_lds_bytes(W, &lcap, &ccap) > lds_bytes || job[5] != lcap) return;
  sample_rows_yuv(reinterpret_cast<const uint8_t*>(job[0]), job[1], 0, frame, H, W, yuv_tight(H, W), params + 5 * j, false, arena, slot,
                  0, 1, S, lcap, ccap, layout, k, mean, inv_std, lds);
}

// the host copy of an ingest job table: every row as csts_stream_ingest asks it of its chunk -> the widest row's LDS bytes, or -1
int group_ingest_check(const int64_t* jobs_host, int njobs, const void* jobs, const void* params, const void* pairs, int npairs,
                       const void* arena, int64_t arena_slots, int S, const float* mean, const float* std, bool yuv) {
  CSTS_REQUIRE(jobs_host && njobs > 0 && njobs <= 65535, "the host copy of the job table is missing, or 1 <= njobs <= 65535 fails");
  CSTS_REQUIRE(npairs > 0 && npairs <= 65535 && arena_slots > 0 && S > 0 && S <= 4096 &&
                   arena_slots * 3 * S * S < ((int64_t)1 << 40) && arena_slots < ((int64_t)1 << 31),
               "bad sizes (S <= 4096, 1 <= pairs <= 65535)");
  int lds = 0;
  for (int j = 0; j < njobs; ++j) {
    const int64_t* job = jobs_host + (int64_t)j * GROUP_INGEST_JOB;
    const int64_t bytes = job[1], K = job[2], H = job[3], W = job[4];
    CSTS_REQUIRE(job[0] != 0 && K > 0 && K < ((int64_t)1 << 31) && H > 0 && H < ((int64_t)1 << 31) && W > 0 && W <= 6000,
                 "a job has a null chunk or bad sizes (K, H >= 1, 1 <= W <= 6000)");
    CSTS_REQUIRE((job[0] & 15) == 0, "every chunk must be 16-byte aligned");
    int cap, ccap, need;
    if (yuv) {
      CSTS_REQUIRE(H >= 2 && W >= 2 && (H & 1) == 0 && (W & 1) == 0, "4:2:0 frames need even H, W >= 2");
      CSTS_REQUIRE(bytes == K * yuv_frame_bytes((int)H, (int)W), "a job's chunk bytes are not K * H * 3 / 2 * W");
      need = sample_yuv_lds_bytes((int)W, &cap, &ccap);
    } else {
      CSTS_REQUIRE(bytes == K * H * W * 3, "a job's chunk bytes are not K * H * W * 3");
      need = sample_lds_bytes((int)W, &cap);
    }
    CSTS_REQUIRE(job[5] == cap, "a job's LDS row capacity is not the one its W asks for");
    lds = std::max(lds, need);
  }
  CSTS_REQUIRE(jobs && params && pairs && arena && mean && std, "bad args");
  CSTS_REQUIRE(aligned16(arena), "the arena must be 16-byte aligned");
  return lds;
}

}  // namespace

extern "C" int csts_stream_stft(const float* buf, int64_t s_base, int64_t m, int64_t n_total, int64_t f0, int64_t f1, float* ring,
                                int ring_cols, int n_fft, int hop, int win, float eps, hipStream_t stream) {
  CSTS_REQUIRE(ring && (buf || m == 0) && m >= 0 && s_base >= 0 && n_fft > 0 && hop > 0 && win > 0 && win <= n_fft && n_fft <= 2048,
               "bad args");
  CSTS_REQUIRE(f0 >= 0 && f1 > f0 && ring_cols > 0 && f1 - f0 <= ring_cols && f1 <= ((int64_t)1 << 40),
               "columns [f0, f1) must be non-empty and at most one turn of the ring");
  CSTS_REQUIRE(n_total < 0 || n_total <= s_base + m, "n_total lies past the samples pushed");
  // every sample a column reads is zero by rule (before 0, at or past n_total) or inside the buffer
  const int64_t first = std::max<int64_t>(stft_first_sample(f0, n_fft, hop, win), 0);
  int64_t last = stft_first_sample(f1 - 1, n_fft, hop, win) + win;          // one past the last sample read
  if (n_total >= 0) last = std::min(last, n_total);
  CSTS_REQUIRE(last <= first || (first >= s_base && last <= s_base + m), "a column needs a sample the buffer does not hold");
  const size_t sm = (size_t)stft_lds_floats(n_fft, win) * sizeof(float);
  hipLaunchKernelGGL(stream_stft_kernel, dim3((unsigned)(f1 - f0)), dim3(256), sm, stream, buf, s_base, m, n_total, f0, ring,
                     ring_cols, n_fft, hop, win, eps);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_stream_audio_windows(const float* ring, int ring_cols, int64_t newest, const int64_t* centers, float* out, int B,
                                         int T, int nbins, int width, hipStream_t stream) {
  CSTS_REQUIRE(ring && centers && out && B > 0 && T > 0 && nbins > 0 && width > 0 && (int64_t)B * T <= 65535,
               "bad args (B * T <= 65535)");
  CSTS_REQUIRE((width & 1) == 0 && width <= ring_cols, "width must be even and at most ring_cols");
  const bool vec = (width & 3) == 0 && aligned16(out);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv((int64_t)nbins * width, vec ? 1024 : 256), 1024), B * T);
  if (vec)
    hipLaunchKernelGGL(stream_audio_windows_kernel<true>, grid, dim3(256), 0, stream, ring, ring_cols, newest, centers, out, nbins,
                       width);
  else
    hipLaunchKernelGGL(stream_audio_windows_kernel<false>, grid, dim3(256), 0, stream, ring, ring_cols, newest, centers, out, nbins,
                       width);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_stream_ingest(const uint8_t* chunk_khwc, int K, int H, int W, const int* pairs, int npairs, const int* params,
                                  float* ring, int R, int S, const float mean[3], const float std[3], hipStream_t stream) {
  if (ingest_check(chunk_khwc, pairs, params, ring, mean, std, K, H, W, npairs, R, S)) return -1;
  int rowcap;
  const int lds = sample_lds_bytes(W, &rowcap);
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&stream_ingest_kernel), lds), "LDS opt-in");
  const float3 m = make_float3(mean[0], mean[1], mean[2]), is = make_float3(1.f / std[0], 1.f / std[1], 1.f / std[2]);
  hipLaunchKernelGGL(stream_ingest_kernel, dim3((unsigned)cdiv(S, SAMPLE_ROWS), npairs), dim3(256), lds, stream, chunk_khwc, K, H, W,
                     pairs, params, ring, R, S, (int64_t)K * H * W * 3, rowcap, m, is);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_stream_ingest_yuv_win(const uint8_t* chunk_yuv, int K, int H, int W, int Hs, int Ws, int top, int left,
                                          const int* pairs, int npairs, const int* params, float* ring, int R, int S,
                                          const float mean[3], const float std[3], int layout, int matrix, int full_range,
                                          hipStream_t stream) {
  if (ingest_check(chunk_yuv, pairs, params, ring, mean, std, K, H, W, npairs, R, S)) return -1;
  CSTS_REQUIRE(yuv_args_ok(layout, matrix), "layout must be CSTS_YUV_NV12 or CSTS_YUV_I420, matrix CSTS_YUV_BT601 or CSTS_YUV_BT709");
  CSTS_REQUIRE(H >= 2 && W >= 2 && (H & 1) == 0 && (W & 1) == 0, "4:2:0 frames need even H, W >= 2");
  const YuvSurf sf = {Hs, Ws, top, left};
  CSTS_REQUIRE(yuv_surf_ok(H, W, sf), YUV_SURF_MSG);
  int lcap, ccap;
  const int lds = sample_yuv_lds_bytes(W, &lcap, &ccap);
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&stream_ingest_yuv_kernel), lds), "LDS opt-in");
  const float3 m = make_float3(mean[0], mean[1], mean[2]), is = make_float3(1.f / std[0], 1.f / std[1], 1.f / std[2]);
  hipLaunchKernelGGL(stream_ingest_yuv_kernel, dim3((unsigned)cdiv(S, SAMPLE_ROWS), npairs), dim3(256), lds, stream, chunk_yuv, K, H, W,
                     sf, pairs, params, ring, R, S, (int64_t)K * yuv_frame_bytes(sf), lcap, ccap, layout, yuv_coef(matrix, full_range),
                     m, is);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_stream_ingest_yuv(const uint8_t* chunk_yuv, int K, int H, int W, const int* pairs, int npairs, const int* params,
                                      float* ring, int R, int S, const float mean[3], const float std[3], int layout, int matrix,
                                      int full_range, hipStream_t stream) {
  return csts_stream_ingest_yuv_win(chunk_yuv, K, H, W, H, W, 0, 0, pairs, npairs, params, ring, R, S, mean, std, layout, matrix,
                                    full_range, stream);
}

extern "C" int csts_stream_gather(const float* ring, int R, const int* slots, float* out, int B, int T, int S, hipStream_t stream) {
  CSTS_REQUIRE(ring && slots && out && R > 0 && B > 0 && B <= 65535 && T > 0 && T <= SPATIAL_MAX_T && S > 0 && S <= 4096,
               "bad args (B <= 65535, T <= 64, S <= 4096)");
  const int64_t plane = (int64_t)S * S;
  const bool vec = (plane & 3) == 0 && aligned16(ring) && aligned16(out);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(plane, vec ? 1024 : 256), 1024), 3 * T, B);
  if (vec)
    hipLaunchKernelGGL(stream_gather_kernel<true>, grid, dim3(256), 0, stream, ring, R, slots, out, T, plane);
  else
    hipLaunchKernelGGL(stream_gather_kernel<false>, grid, dim3(256), 0, stream, ring, R, slots, out, T, plane);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_live_track_add(const float* maps, const int64_t* target_idx, int P, int H, int W, float* sum, int* count,
                                   int64_t* frame, int Rt, hipStream_t stream) {
  CSTS_REQUIRE(maps && target_idx && sum && count && frame, "null maps, target_idx or ring");
  CSTS_REQUIRE(P >= 1 && P <= 65535 && Rt >= 1 && Rt <= 65535, "1 <= P <= 65535 maps, 1 <= Rt <= 65535 slots");
  CSTS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= CSTS_GAZE_DECODE_MAX_HW, "1 <= H * W <= CSTS_GAZE_DECODE_MAX_HW");
  CSTS_REQUIRE((const void*)maps != (const void*)sum, "maps must not be the ring");
  const int hw = H * W;
  const bool vec = hw % 4 == 0 && aligned16(maps) && aligned16(sum);
  if (vec) hipLaunchKernelGGL(live_track_add_kernel<true>, dim3((unsigned)Rt), dim3(256), 0, stream, maps, target_idx, P, hw, sum, count,
                              frame, Rt);
  else hipLaunchKernelGGL(live_track_add_kernel<false>, dim3((unsigned)Rt), dim3(256), 0, stream, maps, target_idx, P, hw, sum, count,
                          frame, Rt);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_live_track_rows(const float* sum, const int* count, const int64_t* frame, int Rt, int64_t f0, int K, int H, int W,
                                    int mode, int max_gap, float* heatmaps, float* rescaled, float* points, float* peak,
                                    int* out_count, int* neighbours, hipStream_t stream) {
  CSTS_REQUIRE(sum && count && frame, "null ring");
  CSTS_REQUIRE(Rt >= 1 && Rt <= 65535 && K >= 1 && K <= 65535, "1 <= Rt <= 65535 slots, 1 <= K <= 65535 frames");
  CSTS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= CSTS_GAZE_DECODE_MAX_HW, "1 <= H * W <= CSTS_GAZE_DECODE_MAX_HW (the frame is held in registers)");
  CSTS_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (hold) or 1 (linear)");
  CSTS_REQUIRE(max_gap >= 1 && max_gap <= CSTS_GAZE_FILL_MAX_GAP, "1 <= max_gap <= CSTS_GAZE_FILL_MAX_GAP");
  CSTS_REQUIRE(f0 >= 0 && f0 + K + max_gap < ((int64_t)1 << 31), "0 <= f0 and f0 + K + max_gap < 2^31 (neighbours are int32)");
  CSTS_REQUIRE(heatmaps != sum && rescaled != sum, "no output may be the ring");
  if (!heatmaps && !rescaled && !points && !peak && !out_count && !neighbours) return 0;
  const int hw = H * W;
  const bool vec = hw % 4 == 0 && aligned16(sum) && aligned16(heatmaps) && aligned16(rescaled);
  const int nch = (int)cdiv(hw, 1024);
  static_assert(DEC_MAX_NCH == 8, "the dispatch below covers 1, 2, 4 and 8 chunks per lane");
  const unsigned n = (unsigned)K;
  if (nch <= 1) launch_live_rows<1>(vec, n, stream, sum, count, frame, Rt, f0, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  else if (nch <= 2) launch_live_rows<2>(vec, n, stream, sum, count, frame, Rt, f0, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  else if (nch <= 4) launch_live_rows<4>(vec, n, stream, sum, count, frame, Rt, f0, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  else launch_live_rows<8>(vec, n, stream, sum, count, frame, Rt, f0, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_group_live_add(const float* maps, const int64_t* target_idx, const int* stream_of, int P, int H, int W, float* sum,
                                   int* count, int64_t* frame, int streams, int Rt, hipStream_t stream) {
  CSTS_REQUIRE(P >= 1 && P <= 65535 && Rt >= 1 && Rt <= 65535, "1 <= P <= 65535 maps, 1 <= Rt <= 65535 slots");
  CSTS_REQUIRE(streams >= 1 && streams <= 65535 && (int64_t)streams * Rt < ((int64_t)1 << 31),
               "1 <= streams <= 65535 and streams * Rt < 2^31");
  CSTS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= CSTS_GAZE_DECODE_MAX_HW, "1 <= H * W <= CSTS_GAZE_DECODE_MAX_HW");
  CSTS_REQUIRE(maps && target_idx && stream_of && sum && count && frame, "null maps, target_idx, stream_of or arena");
  CSTS_REQUIRE((const void*)maps != (const void*)sum, "maps must not be the arena");
  const int hw = H * W;
  const bool vec = hw % 4 == 0 && aligned16(maps) && aligned16(sum);
  const dim3 grid((unsigned)Rt, (unsigned)streams);
  if (vec) hipLaunchKernelGGL(group_live_add_kernel<true>, grid, dim3(256), 0, stream, maps, target_idx, stream_of, P, hw, sum, count,
                              frame, Rt);
  else hipLaunchKernelGGL(group_live_add_kernel<false>, grid, dim3(256), 0, stream, maps, target_idx, stream_of, P, hw, sum, count,
                          frame, Rt);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_group_live_rows(const float* sum, const int* count, const int64_t* frame, int streams, int Rt, const int* stream_of,
                                    const int64_t* frame_of, int K, int H, int W, int mode, int max_gap, float* heatmaps,
                                    float* rescaled, float* points, float* peak, int* out_count, int* neighbours, hipStream_t stream) {
  CSTS_REQUIRE(Rt >= 1 && Rt <= 65535 && K >= 1 && K <= 65535, "1 <= Rt <= 65535 slots, 1 <= K <= 65535 frames");
  CSTS_REQUIRE(streams >= 1 && (int64_t)streams * Rt < ((int64_t)1 << 31), "1 <= streams and streams * Rt < 2^31");
  CSTS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= CSTS_GAZE_DECODE_MAX_HW, "1 <= H * W <= CSTS_GAZE_DECODE_MAX_HW (the frame is held in registers)");
  CSTS_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (hold) or 1 (linear)");
  CSTS_REQUIRE(max_gap >= 1 && max_gap <= CSTS_GAZE_FILL_MAX_GAP, "1 <= max_gap <= CSTS_GAZE_FILL_MAX_GAP");
  CSTS_REQUIRE(sum && count && frame && stream_of && frame_of, "null arena, stream_of or frame_of");
  CSTS_REQUIRE(heatmaps != sum && rescaled != sum && (const void*)out_count != (const void*)count &&
                   (const void*)points != (const void*)sum && (const void*)peak != (const void*)sum,
               "no output may be the arena");
  if (!heatmaps && !rescaled && !points && !peak && !out_count && !neighbours) return 0;
  const int hw = H * W;
  const bool vec = hw % 4 == 0 && aligned16(sum) && aligned16(heatmaps) && aligned16(rescaled);
  const int nch = (int)cdiv(hw, 1024);
  static_assert(DEC_MAX_NCH == 8, "the dispatch below covers 1, 2, 4 and 8 chunks per lane");
  const unsigned n = (unsigned)K;
  if (nch <= 1) launch_group_live_rows<1>(vec, n, stream, sum, count, frame, streams, Rt, stream_of, frame_of, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  else if (nch <= 2) launch_group_live_rows<2>(vec, n, stream, sum, count, frame, streams, Rt, stream_of, frame_of, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  else if (nch <= 4) launch_group_live_rows<4>(vec, n, stream, sum, count, frame, streams, Rt, stream_of, frame_of, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  else launch_group_live_rows<8>(vec, n, stream, sum, count, frame, streams, Rt, stream_of, frame_of, H, W, mode, max_gap, heatmaps, rescaled, points, peak, out_count, neighbours);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_group_stft(const int64_t* jobs, const int64_t* jobs_host, int njobs, float* rings, int streams, int ring_cols,
                               int n_fft, int hop, int win, float eps, hipStream_t stream) {
  CSTS_REQUIRE(jobs_host && njobs > 0 && njobs <= 65535, "the host copy of the job table is missing, or 1 <= njobs <= 65535 fails");
  CSTS_REQUIRE(streams > 0 && ring_cols > 0 && n_fft > 0 && hop > 0 && win > 0 && win <= n_fft && n_fft <= 2048, "bad args");
  std::vector<char> named((size_t)streams, 0);
  int64_t total = 0;
  for (int j = 0; j < njobs; ++j) {
    const int64_t* job = jobs_host + (int64_t)j * GROUP_STFT_JOB;
    const int64_t s_base = job[1], m = job[2], n_total = job[3], f0 = job[4], f1 = job[5], slot = job[6];
    CSTS_REQUIRE(slot >= 0 && slot < streams, "a job names a stream outside [0, streams)");
    CSTS_REQUIRE(!named[(size_t)slot], "two jobs name one stream");
    named[(size_t)slot] = 1;
    CSTS_REQUIRE((job[0] != 0 || m == 0) && m >= 0 && s_base >= 0, "a job has a null sample buffer or bad sizes");
    CSTS_REQUIRE(f0 >= 0 && f1 >= f0 && f1 - f0 <= ring_cols && f1 <= ((int64_t)1 << 40),
                 "a job's columns [f0, f1) must be at most one turn of the ring");
    CSTS_REQUIRE(n_total < 0 || n_total <= s_base + m, "n_total lies past the samples pushed");
    CSTS_REQUIRE(job[7] == total, "a job's first workgroup is not the number of columns before it");
    if (f1 > f0) {   // every sample a column reads is zero by rule (before 0, at or past n_total) or inside the job's buffer
      const int64_t first = std::max<int64_t>(stft_first_sample(f0, n_fft, hop, win), 0);
      int64_t last = stft_first_sample(f1 - 1, n_fft, hop, win) + win;        // one past the last sample read
      if (n_total >= 0) last = std::min(last, n_total);
      CSTS_REQUIRE(last <= first || (first >= s_base && last <= s_base + m), "a column needs a sample the buffer does not hold");
    }
    total += f1 - f0;
  }
  CSTS_REQUIRE(total < ((int64_t)1 << 31), "too many columns in one launch");
  if (total == 0) return 0;
  CSTS_REQUIRE(jobs && rings, "bad args");
  const size_t sm = (size_t)stft_lds_floats(n_fft, win) * sizeof(float);
  hipLaunchKernelGGL(group_stft_kernel, dim3((unsigned)total), dim3(256), sm, stream, jobs, njobs, rings, streams, n_fft / 2 + 1,
                     ring_cols, n_fft, hop, win, eps);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_group_audio_windows(const float* rings, int streams, int ring_cols, const int* stream_of, const int64_t* newest,
                                        const int64_t* centers, float* out, int B, int T, int nbins, int width, hipStream_t stream) {
  CSTS_REQUIRE(rings && stream_of && newest && centers && out && streams > 0 && B > 0 && T > 0 && nbins > 0 && width > 0 &&
                   (int64_t)B * T <= 65535, "bad args (B * T <= 65535)");
  CSTS_REQUIRE((width & 1) == 0 && width <= ring_cols, "width must be even and at most ring_cols");
  const bool vec = (width & 3) == 0 && aligned16(out);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv((int64_t)nbins * width, vec ? 1024 : 256), 1024), B * T);
  if (vec)
    hipLaunchKernelGGL(group_audio_windows_kernel<true>, grid, dim3(256), 0, stream, rings, streams, ring_cols, stream_of, newest,
                       centers, out, T, nbins, width);
  else
    hipLaunchKernelGGL(group_audio_windows_kernel<false>, grid, dim3(256), 0, stream, rings, streams, ring_cols, stream_of, newest,
                       centers, out, T, nbins, width);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_group_ingest(const int64_t* jobs, const int64_t* jobs_host, int njobs, const int* params, const int* pairs,
                                 int npairs, float* arena, int64_t arena_slots, int S, const float mean[3], const float std[3],
                                 hipStream_t stream) {
  const int lds = group_ingest_check(jobs_host, njobs, jobs, params, pairs, npairs, arena, arena_slots, S, mean, std, false);
  if (lds < 0) return -1;
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&group_ingest_kernel), lds), "LDS opt-in");
  const float3 m = make_float3(mean[0], mean[1], mean[2]), is = make_float3(1.f / std[0], 1.f / std[1], 1.f / std[2]);
  hipLaunchKernelGGL(group_ingest_kernel, dim3((unsigned)cdiv(S, SAMPLE_ROWS), npairs), dim3(256), lds, stream, jobs, njobs, params,
                     pairs, arena, (int)arena_slots, S, lds, m, is);
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_group_ingest_yuv(const int64_t* jobs, const int64_t* jobs_host, int njobs, const int* params, const int* pairs,
                                     int npairs, float* arena, int64_t arena_slots, int S, const float mean[3], const float std[3],
                                     int layout, int matrix, int full_range, hipStream_t stream) {
  CSTS_REQUIRE(yuv_args_ok(layout, matrix), "layout must be CSTS_YUV_NV12 or CSTS_YUV_I420, matrix CSTS_YUV_BT601 or CSTS_YUV_BT709");
  const int lds = group_ingest_check(jobs_host, njobs, jobs, params, pairs, npairs, arena, arena_slots, S, mean, std, true);
  if (lds < 0) return -1;
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&group_ingest_yuv_kernel), lds), "LDS opt-in");
  const float3 m = make_float3(mean[0], mean[1], mean[2]), is = make_float3(1.f / std[0], 1.f / std[1], 1.f / std[2]);
  hipLaunchKernelGGL(group_ingest_yuv_kernel, dim3((unsigned)cdiv(S, SAMPLE_ROWS), npairs), dim3(256), lds, stream, jobs, njobs, params,
                     pairs, arena, (int)arena_slots, S, lds, layout, yuv_coef(matrix, full_range), m, is);
  CSTS_LAUNCH_CHECK();
  return 0;
}
