// 4:2:0 YUV frames on the device: pictures the way video sources deliver them (NV12 from hardware decoders, I420 from software
// ones), 1.5 bytes per pixel instead of the 3 of packed RGB.  include/csts_hip.h states the layouts and the integer colour rule;
// yuv_pixel (yuv_shared.h) is its one implementation, run on the device by every kernel here and on the host by
// csts_yuv_to_rgb_host; rgb_luma / rgb_chroma are the inverse rule, run by rgb_to_yuv here and by the 4:2:0 overlay (overlay.hip).
//
// yuv_to_rgb: the streaming converter (N, H * 3 / 2, W) -> (N, H, W, 3) for the consumers that draw RGB (the overlay renderers).
// A workgroup owns one pair of luma rows of one tile of YUV_TW pixels and the chroma they share: it stages those source bytes in
// LDS as 16-byte chunks laid out from the address (a recording and its frames start at any byte), converts pixel pairs into an
// LDS image of the two output rows laid out from the output address (any byte as well: a renderer converts into a chunk of its
// output), and writes that image back as 16-byte chunks (the ragged first and last chunk of a row segment byte by byte: the
// neighbouring workgroup owns the rest of them).
//
// rgb_to_yuv: the way back for the consumers that want 4:2:0 again (an encoder behind the overlay), by the inverse rule of the
// header (rgb_luma / rgb_chroma, yuv_shared.h): the same tiles and the same staging, (N, H, W, 3) -> (N, H * 3 / 2, W).
//
// spatial / clip / batch_sample_yuv: the pixel pass of spatial.hip and batch.hip reading 4:2:0 pictures in place
// (sample_rows_yuv, yuv_shared.h): bit for bit the RGB pass on the converted pictures, without the converted pictures.
//
// Decoder surfaces (the *_win entry points, include/csts_hip.h): the pictures are windows of padded surfaces.  Every kernel takes a
// YuvSurf (yuv_shared.h) next to H, W and forms its addresses from it; a tight picture is the surface {H, W, 0, 0}, so the tight
// entry points are the same launches of the same kernels.
#include "yuv_shared.h"

namespace {

constexpr int YUV_TW = 1024;                     // pixels of one tile of a row pair (even)
constexpr int YUV_INCAP = YUV_TW + 32;           // a staged source span: up to YUV_TW bytes + 30, rounded up to 16
constexpr int YUV_OUTCAP = 3 * YUV_TW + 32;      // the image of one output row segment

// grid (ceil(W / YUV_TW), H / 2, min(N, 65535)), 256 threads.  src is the recording's address rounded DOWN to 16 bytes; the
// recording is the bytes [lo, hi) from there.  out likewise: the output's address rounded down, its first byte olo bytes from there
// (the output may start at any byte as well: a chunk of a larger tensor).  The pictures are the H x W windows of the surfaces sf;
// the output is tight.
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const uint8_t* __restrict__ src, int64_t lo, int64_t hi,
                                                         uint8_t* __restrict__ out, int64_t olo, int64_t N, int H, int W, YuvSurf sf,
                                                         int layout, YuvCoef k) {
  __shared__ __align__(16) uint8_t in[4][YUV_INCAP];
  __shared__ __align__(16) uint8_t img[2][YUV_OUTCAP];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * YUV_TW, tw = min(YUV_TW, W - x0), cy = blockIdx.y;
  const bool nv12 = layout == CSTS_YUV_NV12;
  for (int64_t n = blockIdx.z; n < N; n += gridDim.z) {
    const int64_t f0 = lo + n * yuv_frame_bytes(sf), l0 = f0 + yuv_luma_row(sf, 2 * cy) + x0;
    const int64_t q = f0 + yuv_chroma_row(sf, cy, nv12) + (nv12 ? x0 : x0 >> 1);
    int sh[4];
    sh[0] = yuv_stage(in[0], src, l0, l0 + tw, lo, hi, tid, 256);
    sh[1] = yuv_stage(in[1], src, l0 + sf.Ws, l0 + sf.Ws + tw, lo, hi, tid, 256);
    if (nv12) {
      sh[2] = yuv_stage(in[2], src, q, q + tw, lo, hi, tid, 256);
      sh[3] = sh[2] + 1;
    } else {
      const int64_t q1 = q + yuv_vplane(sf);
      sh[2] = yuv_stage(in[2], src, q, q + (tw >> 1), lo, hi, tid, 256);
      sh[3] = yuv_stage(in[3], src, q1, q1 + (tw >> 1), lo, hi, tid, 256);
    }
    __syncthreads();
    // byte of out where this segment of output row r starts, and where that byte lies in img[r]: even whenever the output's
    // address is (W and x0 are even), and then a pixel pair goes as three 2-byte stores; an odd output goes byte by byte
    int64_t o[2];
    int os[2];
    for (int r = 0; r < 2; ++r) {
      o[r] = olo + (((int64_t)n * H + 2 * cy + r) * W + x0) * 3;
      os[r] = (int)(o[r] & 15);
    }
    const uint8_t* cu = in[2];                                  // nv12: V follows U (sh[3] = sh[2] + 1); i420: a row of its own
    const uint8_t* cv = nv12 ? in[2] : in[3];
    const int cstep = nv12 ? 2 : 1;
    for (int p = tid; p < (tw >> 1); p += 256) {
      const int U = cu[sh[2] + p * cstep], V = cv[sh[3] + p * cstep];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        int R0, G0, B0, R1, G1, B1;
        yuv_pixel(k, in[r][sh[r] + 2 * p], U, V, R0, G0, B0);
        yuv_pixel(k, in[r][sh[r] + 2 * p + 1], U, V, R1, G1, B1);
        uint8_t* d8 = img[r] + os[r] + 6 * p;
        if ((os[r] & 1) == 0) {
          unsigned short* d = reinterpret_cast<unsigned short*>(d8);
          d[0] = (unsigned short)(R0 | (G0 << 8));
          d[1] = (unsigned short)(B0 | (R1 << 8));
          d[2] = (unsigned short)(G1 | (B1 << 8));
        } else {
          d8[0] = (uint8_t)R0; d8[1] = (uint8_t)G0; d8[2] = (uint8_t)B0;
          d8[3] = (uint8_t)R1; d8[4] = (uint8_t)G1; d8[5] = (uint8_t)B1;
        }
      }
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
      const int beg = os[r], end = os[r] + 3 * tw;              // the bytes of img[r] this workgroup owns
      uint8_t* g = out + (o[r] - os[r]);                        // 16-byte aligned
      for (int c = tid * 16; c < end; c += 256 * 16) {
        if (c >= beg && c + 16 <= end) {
          *reinterpret_cast<uint4*>(g + c) = *reinterpret_cast<const uint4*>(img[r] + c);
        } else {
          for (int q = 0; q < 16; ++q)
            if (c + q >= beg && c + q < end) g[c + q] = img[r][c + q];
        }
      }
    }
    __syncthreads();                                            // the next frame reuses in[] and img[]
  }
}

// rgb_to_yuv, the way back (rgb_luma / rgb_chroma, yuv_shared.h), with the staging of yuv_to_rgb_kernel turned round: a workgroup
// owns the same row pair of the same tile, stages its 2 x 3 tw RGB bytes, and builds LDS images of the two luma segments and of
// the chroma segment(s) (nv12: one interleaved, i420: one of U and one of V), each laid out from its output address.
// grid (ceil(W / YUV_TW), H / 2, min(N, 65535)), 256 threads; src, lo, hi, out, olo as above.
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const uint8_t* __restrict__ src, int64_t lo, int64_t hi,
                                                         uint8_t* __restrict__ out, int64_t olo, int64_t N, int H, int W, int layout,
                                                         RgbCoef k) {
  __shared__ __align__(16) uint8_t in[2][YUV_OUTCAP];
  __shared__ __align__(16) uint8_t img[4][YUV_INCAP];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * YUV_TW, tw = min(YUV_TW, W - x0), cy = blockIdx.y, hw = W >> 1;
  const bool nv12 = layout == CSTS_YUV_NV12;
  const int nspans = nv12 ? 3 : 4;
  for (int64_t n = blockIdx.z; n < N; n += gridDim.z) {
    const int64_t r0 = lo + (((int64_t)n * H + 2 * cy) * W + x0) * 3;
    int sh[2];
    sh[0] = yuv_stage(in[0], src, r0, r0 + 3 * tw, lo, hi, tid, 256);
    sh[1] = yuv_stage(in[1], src, r0 + (int64_t)W * 3, r0 + (int64_t)W * 3 + 3 * tw, lo, hi, tid, 256);
    __syncthreads();
    // the four output segments: where each starts in out, how long it is, and where its first byte lies in its image
    const int64_t f0 = olo + n * yuv_frame_bytes(H, W), c0 = f0 + (int64_t)H * W;
    int64_t o[4];
    int os[4], len[4];
    o[0] = f0 + (int64_t)(2 * cy) * W + x0;
    o[1] = o[0] + W;
    o[2] = nv12 ? c0 + (int64_t)cy * W + x0 : c0 + (int64_t)cy * hw + (x0 >> 1);
    o[3] = o[2] + (int64_t)(H >> 1) * hw;
    len[0] = len[1] = tw;
    len[2] = nv12 ? tw : tw >> 1;
    len[3] = tw >> 1;
    for (int s = 0; s < 4; ++s) os[s] = (int)(o[s] & 15);
    for (int p = tid; p < (tw >> 1); p += 256) {
      int SR = 0, SG = 0, SB = 0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const uint8_t* s = in[r] + sh[r] + 6 * p;
        const int R0 = s[0], G0 = s[1], B0 = s[2], R1 = s[3], G1 = s[4], B1 = s[5];
        img[r][os[r] + 2 * p] = (uint8_t)rgb_luma(k, R0, G0, B0);
        img[r][os[r] + 2 * p + 1] = (uint8_t)rgb_luma(k, R1, G1, B1);
        SR += R0 + R1;
        SG += G0 + G1;
        SB += B0 + B1;
      }
      int U, V;
      rgb_chroma(k, SR, SG, SB, U, V);
      if (nv12) {
        img[2][os[2] + 2 * p] = (uint8_t)U;
        img[2][os[2] + 2 * p + 1] = (uint8_t)V;
      } else {
        img[2][os[2] + p] = (uint8_t)U;
        img[3][os[3] + p] = (uint8_t)V;
      }
    }
    __syncthreads();
    for (int s = 0; s < nspans; ++s) yuv_unstage(out + (o[s] - os[s]), img[s], os[s], os[s] + len[s], tid, 256);
    __syncthreads();                                            // the next frame reuses in[] and img[]
  }
}

// row b of the clip table {byte offset, N, H, W} of 4:2:0 recordings (H the luma height): H, W even, the N H W 3 / 2 bytes lie inside
// [0, arena_bytes) and a row fits the staged LDS
__device__ __forceinline__ bool clip_row_ok_yuv(const int64_t* __restrict__ row, int64_t arena_bytes, int max_W) {
  const int64_t off = row[0], N = row[1], H = row[2], W = row[3];
  if (off < 0 || off > arena_bytes || N < 1 || H < 2 || W < 2 || W > max_W || H > 0x7fffffff || N > 0x7fffffff) return false;
  if ((H | W) & 1) return false;
  return N <= (arena_bytes - off) / yuv_frame_bytes(H, W);   // H W 3 / 2 < 2^45: no overflow; N H W 3 / 2 is never formed
}

// grid (ceil(S / 4), T, B), 256 threads; dynamic LDS: sample_yuv_lds_bytes.
// INDEXED: src is a video of nsrc frames and frames_idx [B][T] names the frame of each (b, t); otherwise frame (b, t) is b * T + t.
// The pictures are the H x W windows of the surfaces sf.
template <bool INDEXED>
__global__ __launch_bounds__(256) void sample_yuv_kernel(const uint8_t* __restrict__ src, const int* __restrict__ frames_idx,
                                                         int64_t nsrc, const int* __restrict__ params, float* __restrict__ out, int T,
                                                         int H, int W, YuvSurf sf, int S, int64_t src_bytes, int lcap, int ccap, int layout,
                                                         YuvCoef k, float3 mean, float3 inv_std) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int t = blockIdx.y, b = blockIdx.z;
  int64_t frame = (int64_t)b * T + t;
  if (INDEXED) frame = min(max((int64_t)frames_idx[frame], (int64_t)0), nsrc - 1);     // as temporal_sampling clamps
  sample_rows_yuv(src, src_bytes, 0, frame, H, W, sf, params + 5 * b, false, out, b, t, T, S, lcap, ccap, layout, k, mean, inv_std, lds);
}

__global__ __launch_bounds__(256) void batch_sample_yuv_kernel(const uint8_t* __restrict__ arena, int64_t arena_bytes,
                                                               const int64_t* __restrict__ clips, const int* __restrict__ frames_idx,
                                                               const int* __restrict__ params, float* __restrict__ out, int T, int S,
                                                               int max_W, int lcap, int ccap, int layout, YuvCoef k, float3 mean,
                                                               float3 inv_std) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int t = blockIdx.y, b = blockIdx.z;
  const int64_t* row = clips + 4 * b;
  const bool ok = clip_row_ok_yuv(row, arena_bytes, max_W);   // uniform over the workgroup (one clip)
  int64_t frame = 0;
  if (ok) frame = min(max((int64_t)frames_idx[(int64_t)b * T + t], (int64_t)0), row[1] - 1);     // as temporal_sampling clamps
  const int H = ok ? (int)row[2] : 2, W = ok ? (int)row[3] : 2;
  sample_rows_yuv(arena, arena_bytes, ok ? row[0] : 0, frame, H, W, yuv_tight(H, W), params + 5 * b, !ok, out, b, t, T, S, lcap, ccap,
                  layout, k, mean, inv_std, lds);
}

template <bool INDEXED>
int launch_sample_yuv(const uint8_t* src, const int* frames_idx, int64_t nsrc, const int* params, float* out, int B, int T, int H,
                      int W, const YuvSurf& sf, int S, const float mean[3], const float std[3], int layout, int matrix, int full_range,
                      hipStream_t stream) {
  int lcap, ccap;
  const int lds = sample_yuv_lds_bytes(W, &lcap, &ccap);
  if (lds > 65536)
    CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&sample_yuv_kernel<INDEXED>), lds), "LDS opt-in");
  const float3 m = make_float3(mean[0], mean[1], mean[2]), is = make_float3(1.f / std[0], 1.f / std[1], 1.f / std[2]);
  const int64_t src_bytes = nsrc * yuv_frame_bytes(sf);
  hipLaunchKernelGGL(sample_yuv_kernel<INDEXED>, dim3((unsigned)cdiv(S, SAMPLE_ROWS), T, B), dim3(256), lds, stream, src, frames_idx,
                     nsrc, params, out, T, H, W, sf, S, src_bytes, lcap, ccap, layout, yuv_coef(matrix, full_range), m, is);
  CSTS_LAUNCH_CHECK();
  return 0;
}

int yuv_frame_check(int64_t N, int H, int W, int layout, int matrix) {
  CSTS_REQUIRE(yuv_args_ok(layout, matrix), "layout must be CSTS_YUV_NV12 or CSTS_YUV_I420, matrix CSTS_YUV_BT601 or CSTS_YUV_BT709");
  CSTS_REQUIRE(N >= 1 && H >= 2 && W >= 2 && (H & 1) == 0 && (W & 1) == 0, "4:2:0 frames need N >= 1 and even H, W >= 2");
  return 0;
}

// csts_yuv_to_rgb(_win) once the window is known to lie in its surface
int yuv_to_rgb_run(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, const YuvSurf& sf, int layout, int matrix,
                   int full_range, hipStream_t stream) {
  CSTS_REQUIRE(frames_yuv && out_nhwc, "bad args");
  if (yuv_frame_check(N, H, W, layout, matrix)) return -1;
  CSTS_REQUIRE(H <= 131070 && N <= ((int64_t)1 << 62) / ((int64_t)sf.Hs * sf.Ws * 3), "bad sizes (H <= 131070)");
  const int64_t lo = (int64_t)(reinterpret_cast<uintptr_t>(frames_yuv) & 15), bytes = N * yuv_frame_bytes(sf);
  const int64_t olo = (int64_t)(reinterpret_cast<uintptr_t>(out_nhwc) & 15);
  const uint8_t* a = frames_yuv, *o = out_nhwc;
  CSTS_REQUIRE(a + bytes <= o || o + N * H * W * 3 <= a, "the output must not overlap the input");
  hipLaunchKernelGGL(yuv_to_rgb_kernel, dim3((unsigned)cdiv(W, YUV_TW), H / 2, (unsigned)std::min<int64_t>(N, 65535)), dim3(256), 0,
                     stream, frames_yuv - lo, lo, lo + bytes, out_nhwc - olo, olo, N, H, W, sf, layout,
                     yuv_coef(matrix, full_range));
  CSTS_LAUNCH_CHECK();
  return 0;
}

int yuv_to_rgb_host_run(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, const YuvSurf& sf, int layout,
                        int matrix, int full_range) {
  CSTS_REQUIRE(frames_yuv && out_nhwc, "bad args");
  if (yuv_frame_check(N, H, W, layout, matrix)) return -1;
  const YuvCoef k = yuv_coef(matrix, full_range);
  const bool nv12 = layout == CSTS_YUV_NV12;
  const int64_t fb = yuv_frame_bytes(sf), vplane = yuv_vplane(sf);
  for (int64_t n = 0; n < N; ++n) {
    const uint8_t* f = frames_yuv + n * fb;
    uint8_t* o = out_nhwc + n * H * W * 3;
    for (int y = 0; y < H; ++y) {
      const uint8_t* l = f + yuv_luma_row(sf, y);
      const uint8_t* c = f + yuv_chroma_row(sf, y >> 1, nv12);
      for (int x = 0; x < W; ++x) {
        const int cx = x >> 1;
        const int U = nv12 ? c[2 * cx] : c[cx];
        const int V = nv12 ? c[2 * cx + 1] : c[vplane + cx];
        int R, G, B;
        yuv_pixel(k, l[x], U, V, R, G, B);
        uint8_t* d = o + ((int64_t)y * W + x) * 3;
        d[0] = (uint8_t)R;
        d[1] = (uint8_t)G;
        d[2] = (uint8_t)B;
      }
    }
  }
  return 0;
}

}  // namespace

extern "C" int csts_yuv_to_rgb(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, int layout, int matrix,
                               int full_range, hipStream_t stream) {
  return yuv_to_rgb_run(frames_yuv, out_nhwc, N, H, W, yuv_tight(H, W), layout, matrix, full_range, stream);
}

extern "C" int csts_yuv_to_rgb_win(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, int Hs, int Ws, int top,
                                   int left, int layout, int matrix, int full_range, hipStream_t stream) {
  const YuvSurf sf = {Hs, Ws, top, left};
  CSTS_REQUIRE(yuv_surf_ok(H, W, sf), YUV_SURF_MSG);
  return yuv_to_rgb_run(frames_yuv, out_nhwc, N, H, W, sf, layout, matrix, full_range, stream);
}

extern "C" int csts_yuv_to_rgb_host(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, int layout, int matrix,
                                    int full_range) {
  return yuv_to_rgb_host_run(frames_yuv, out_nhwc, N, H, W, yuv_tight(H, W), layout, matrix, full_range);
}

extern "C" int csts_yuv_to_rgb_win_host(const uint8_t* frames_yuv, uint8_t* out_nhwc, int64_t N, int H, int W, int Hs, int Ws, int top,
                                        int left, int layout, int matrix, int full_range) {
  const YuvSurf sf = {Hs, Ws, top, left};
  CSTS_REQUIRE(yuv_surf_ok(H, W, sf), YUV_SURF_MSG);
  return yuv_to_rgb_host_run(frames_yuv, out_nhwc, N, H, W, sf, layout, matrix, full_range);
}

extern "C" int csts_rgb_to_yuv(const uint8_t* frames_nhwc, uint8_t* out_yuv, int64_t N, int H, int W, int layout, int matrix,
                               int full_range, hipStream_t stream) {
  CSTS_REQUIRE(frames_nhwc && out_yuv, "bad args");
  if (yuv_frame_check(N, H, W, layout, matrix)) return -1;
  CSTS_REQUIRE(H <= 131070 && N <= ((int64_t)1 << 62) / ((int64_t)H * W * 3), "bad sizes (H <= 131070)");
  const int64_t lo = (int64_t)(reinterpret_cast<uintptr_t>(frames_nhwc) & 15), bytes = N * H * W * 3;
  const int64_t olo = (int64_t)(reinterpret_cast<uintptr_t>(out_yuv) & 15);
  const uint8_t* a = frames_nhwc, *o = out_yuv;
  CSTS_REQUIRE(a + bytes <= o || o + N * yuv_frame_bytes(H, W) <= a, "the output must not overlap the input");
  hipLaunchKernelGGL(rgb_to_yuv_kernel, dim3((unsigned)cdiv(W, YUV_TW), H / 2, (unsigned)std::min<int64_t>(N, 65535)), dim3(256), 0,
                     stream, frames_nhwc - lo, lo, lo + bytes, out_yuv - olo, olo, N, H, W, layout, rgb_coef(matrix, full_range));
  CSTS_LAUNCH_CHECK();
  return 0;
}

extern "C" int csts_rgb_to_yuv_host(const uint8_t* frames_nhwc, uint8_t* out_yuv, int64_t N, int H, int W, int layout, int matrix,
                                    int full_range) {
  CSTS_REQUIRE(frames_nhwc && out_yuv, "bad args");
  if (yuv_frame_check(N, H, W, layout, matrix)) return -1;
  const RgbCoef k = rgb_coef(matrix, full_range);
  const int64_t fb = yuv_frame_bytes(H, W), hw = W / 2;
  for (int64_t n = 0; n < N; ++n) {
    const uint8_t* f = frames_nhwc + n * H * W * 3;
    uint8_t* o = out_yuv + n * fb;
    uint8_t* c = o + (int64_t)H * W;
    for (int cy = 0; cy < H / 2; ++cy) {
      for (int cx = 0; cx < hw; ++cx) {
        int SR = 0, SG = 0, SB = 0;
        for (int dy = 0; dy < 2; ++dy) {
          for (int dx = 0; dx < 2; ++dx) {
            const int64_t px = (int64_t)(2 * cy + dy) * W + 2 * cx + dx;
            const int R = f[3 * px], G = f[3 * px + 1], B = f[3 * px + 2];
            o[px] = (uint8_t)rgb_luma(k, R, G, B);
            SR += R;
            SG += G;
            SB += B;
          }
        }
        int U, V;
        rgb_chroma(k, SR, SG, SB, U, V);
        if (layout == CSTS_YUV_NV12) {
          c[(int64_t)cy * W + 2 * cx] = (uint8_t)U;
          c[(int64_t)cy * W + 2 * cx + 1] = (uint8_t)V;
        } else {
          c[cy * hw + cx] = (uint8_t)U;
          c[(H / 2) * hw + cy * hw + cx] = (uint8_t)V;
        }
      }
    }
  }
  return 0;
}

extern "C" int csts_spatial_sample_yuv_win(const uint8_t* frames_yuv, const int* params, float* out, int B, int T, int H, int W,
                                           int Hs, int Ws, int top, int left, int S, const float mean[3], const float std[3],
                                           int layout, int matrix, int full_range, hipStream_t stream) {
  CSTS_REQUIRE(frames_yuv && params && out && mean && std, "bad args");
  if (yuv_frame_check(1, H, W, layout, matrix)) return -1;
  const YuvSurf sf = {Hs, Ws, top, left};
  CSTS_REQUIRE(yuv_surf_ok(H, W, sf), YUV_SURF_MSG);
  CSTS_REQUIRE(B > 0 && T > 0 && S > 0 && S <= 4096 && W <= 6000 && B <= 65535 && T <= 65535, "bad sizes (W <= 6000, S <= 4096)");
  CSTS_REQUIRE(aligned16(frames_yuv) && aligned16(out), "frames and output must be 16-byte aligned");
  return launch_sample_yuv<false>(frames_yuv, nullptr, (int64_t)B * T, params, out, B, T, H, W, sf, S, mean, std, layout, matrix,
                                  full_range, stream);
}

extern "C" int csts_spatial_sample_yuv(const uint8_t* frames_yuv, const int* params, float* out, int B, int T, int H, int W, int S,
                                       const float mean[3], const float std[3], int layout, int matrix, int full_range,
                                       hipStream_t stream) {
  return csts_spatial_sample_yuv_win(frames_yuv, params, out, B, T, H, W, H, W, 0, 0, S, mean, std, layout, matrix, full_range, stream);
}

extern "C" int csts_clip_sample_yuv_win(const uint8_t* video_yuv, int64_t N, const int* frames_idx, const int* params, float* out,
                                        int B, int T, int H, int W, int Hs, int Ws, int top, int left, int S, const float mean[3],
                                        const float std[3], int layout, int matrix, int full_range, hipStream_t stream) {
  CSTS_REQUIRE(video_yuv && frames_idx && params && out && mean && std, "bad args");
  if (yuv_frame_check(N, H, W, layout, matrix)) return -1;
  const YuvSurf sf = {Hs, Ws, top, left};
  CSTS_REQUIRE(yuv_surf_ok(H, W, sf), YUV_SURF_MSG);
  CSTS_REQUIRE(B > 0 && T > 0 && T <= SPATIAL_MAX_T && S > 0 && S <= 4096 && W <= 6000 && B <= 65535,
               "bad sizes (T <= 64, W <= 6000, S <= 4096)");
  CSTS_REQUIRE(aligned16(video_yuv) && aligned16(out), "video and output must be 16-byte aligned");
  return launch_sample_yuv<true>(video_yuv, frames_idx, N, params, out, B, T, H, W, sf, S, mean, std, layout, matrix, full_range,
                                 stream);
}

extern "C" int csts_clip_sample_yuv(const uint8_t* video_yuv, int64_t N, const int* frames_idx, const int* params, float* out, int B,
                                    int T, int H, int W, int S, const float mean[3], const float std[3], int layout, int matrix,
                                    int full_range, hipStream_t stream) {
  return csts_clip_sample_yuv_win(video_yuv, N, frames_idx, params, out, B, T, H, W, H, W, 0, 0, S, mean, std, layout, matrix,
                                  full_range, stream);
}

extern "C" int csts_batch_sample_yuv(const uint8_t* arena_u8, int64_t arena_bytes, const int64_t* clips, const int* frames_idx,
                                     const int* params, float* out, int B, int T, int S, int max_W, const float mean[3],
                                     const float std[3], int layout, int matrix, int full_range, hipStream_t stream) {
  CSTS_REQUIRE(arena_u8 && clips && frames_idx && params && out && mean && std, "bad args");
  CSTS_REQUIRE(yuv_args_ok(layout, matrix), "layout must be CSTS_YUV_NV12 or CSTS_YUV_I420, matrix CSTS_YUV_BT601 or CSTS_YUV_BT709");
  CSTS_REQUIRE(arena_bytes >= 6 && B > 0 && B <= 65535 && T > 0 && T <= SPATIAL_MAX_T && S > 0 && S <= 4096 && max_W > 0 &&
                   max_W <= 6000, "bad sizes (T <= 64, max_W <= 6000, S <= 4096)");
  CSTS_REQUIRE(aligned16(arena_u8) && aligned16(out), "arena and output must be 16-byte aligned");
  int lcap, ccap;
  const int lds = sample_yuv_lds_bytes(max_W, &lcap, &ccap);
  if (lds > 65536) CSTS_REQUIRE(csts_dyn_lds_optin(reinterpret_cast<const void*>(&batch_sample_yuv_kernel), lds), "LDS opt-in");
  const float3 m = make_float3(mean[0], mean[1], mean[2]), is = make_float3(1.f / std[0], 1.f / std[1], 1.f / std[2]);
  hipLaunchKernelGGL(batch_sample_yuv_kernel, dim3((unsigned)cdiv(S, SAMPLE_ROWS), T, B), dim3(256), lds, stream, arena_u8, arena_bytes,
                     clips, frames_idx, params, out, T, S, max_W, lcap, ccap, layout, yuv_coef(matrix, full_range), m, is);
  CSTS_LAUNCH_CHECK();
  return 0;
}
