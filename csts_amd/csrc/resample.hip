// Audio at any sample rate (csts_amd/inputs.py::resample_audio): rational-ratio band-limited resampling of a waveform to the
// model's rate, the step the reference does offline (data/preprocess.py::extract_audio, ffmpeg -ar 24000 -ac 1).  Polyphase
// form of include/csts_hip.h's rule: the zero-stuffed signal is never built, each output walks only the taps that meet a sample.
//
//   y[m] = sum_i x[i] * h[half + m * down - i * up],   ceil((m down - half) / up) <= i <= floor((m down + half) / up), 0 <= i < n
//
// One output per lane; a workgroup owns runs of CSTS_RESAMPLE_RUN consecutive outputs (run r, r + gridDim.x, ...) and stages per run
// the input span those outputs read in LDS -- coalesced, with the channel mean and the int16 scale applied on the way in, so
// the downmix needs no pass of its own.  The taps are copied to LDS once per workgroup, phase-major: with c = half + m down,
// lane m reads h[(c / up - i) up + c % up], so row c % up of a (up, taps per phase) table holds its taps contiguously, walked
// backwards as i grows.  Rows are an odd number of floats apart so lanes of neighbouring phases start on different banks; the
// staged samples are skewed by one float every 32 (sw) so a decimating ratio (lanes `down / up` samples apart: 8 at 192 kHz)
// does not put every fourth lane on one bank.  All positions are 64-bit: m * down passes 2^31 within an hour of 192 kHz audio.
//
// A live stream (csts_resample_stream, inputs.StreamResampler) runs the same kernel body on a buffer that holds only the samples
// [x_base, x_base + n) of the stream and asks for the outputs [m_first, m_end): the positions stay those of the stream, only the
// addresses are taken relative to x_base and m_first.  For csts_resample_wav both are 0, so an output has the same sum, term by term,
// whichever entry computes it and whichever run it falls in.
#include "common.h"

namespace {

constexpr int RUN = CSTS_RESAMPLE_RUN;

// taps per phase, the row pitch of the phase-major table, and the longest input span one run reads
inline int64_t phase_taps(int64_t up, int64_t half) { return (2 * half + up) / up; }             // ceil((2 half + 1) / up)
inline int64_t span_cap(int64_t up, int64_t down, int64_t half) { return ((RUN - 1) * down + 2 * half) / up + 2; }
inline int64_t skewed(int64_t floats) { return floats + floats / 32 + 1; }

__device__ __forceinline__ int sw(int j) { return j + (j >> 5); }
__device__ __forceinline__ int64_t ceil_div(int64_t a, int64_t b) { return a <= 0 ? -((-a) / b) : (a + b - 1) / b; }     // b > 0

__device__ __forceinline__ float wav_load(const float* p) { return *p; }
__device__ __forceinline__ float wav_load(const int16_t* p) { return (float)*p * (1.0f / 32768.0f); }

// grid (min(runs, 2048), B), 256 threads, dynamic LDS: [up * pstride] taps, [skewed(cap)] samples.  wav (B, C, n) holds the
// stream positions [x_base, x_base + n); out (B, m_end - m_first) receives the outputs [m_first, m_end); no read leaves the buffer.
// STREAM false: a whole waveform, the two offsets are the constant 0 and fold away (csts_resample_wav's code is what it was).
template <typename TIn, bool STREAM>
__global__ __launch_bounds__(256) void resample_kernel(const TIn* __restrict__ wav, int C, int64_t n, int64_t x_base_,
                                                       const float* __restrict__ taps, int up, int down, int half, int P, int pstride,
                                                       int cap, int64_t m_first_, int64_t m_end, int64_t nruns, float* __restrict__ out) {
  const int64_t x_base = STREAM ? x_base_ : 0, m_first = STREAM ? m_first_ : 0;
  extern __shared__ float sm[];
  float* tp = sm;
  float* xs = sm + up * pstride;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  for (int idx = tid; idx < up * pstride; idx += 256) {
    const int p = idx / pstride, q = idx - p * pstride;
    const int64_t t = (int64_t)q * up + p;
    tp[idx] = (q < P && t <= 2 * (int64_t)half) ? taps[t] : 0.f;
  }
  const TIn* x = wav + b * C * n;
  const int64_t lim = x_base + n;                                     // positions are the stream's; reads stay in [x_base, lim)
  for (int64_t run = blockIdx.x; run < nruns; run += gridDim.x) {
    const int64_t m0 = m_first + run * RUN, m1 = min(m0 + RUN, m_end) - 1;
    const int64_t base = max(ceil_div(m0 * down - half, up), x_base);
    const int64_t end = min((m1 * down + half) / up, lim - 1);
    const int span = (int)min(end - base + 1, (int64_t)cap);          // <= cap by the rule; the clamp keeps a bad call inside LDS
    __syncthreads();                                                  // the taps are in; the previous run is done with xs
    for (int j = tid; j < span; j += 256) {
      const int64_t at = base - x_base + j;
      float s = wav_load(x + at);
      for (int c = 1; c < C; ++c) s += wav_load(x + c * n + at);
      xs[sw(j)] = C > 1 ? s / (float)C : s;
    }
    __syncthreads();
    const int64_t m = m0 + tid;
    if (m <= m1) {
      const int64_t cpos = m * down + half;                           // the tap index that meets sample 0
      const int64_t qc = cpos / up;
      const float* row = tp + (int)(cpos - qc * up) * pstride;
      const int64_t lo = max(ceil_div(cpos - 2 * (int64_t)half, up), base);
      const int64_t hi = min(min(qc, lim - 1), base + span - 1);
      int j = (int)(lo - base), q = (int)(qc - lo);
      float acc = 0.f;
      for (int64_t i = lo; i <= hi; ++i, ++j, --q) acc += xs[sw(j)] * row[q];
      out[b * (m_end - m_first) + (m - m_first)] = acc;
    }
  }
}

}  // namespace

extern "C" int64_t csts_resample_len(int64_t n, int up, int down) {
  if (n < 1 || n > CSTS_RESAMPLE_MAX_N || up < 1 || down < 1 || up > CSTS_RESAMPLE_MAX_RATIO || down > CSTS_RESAMPLE_MAX_RATIO) return -1;
  return (n * up + down - 1) / down;
}

extern "C" int csts_resample_wav(const void* wav, int in_kind, int B, int C, int64_t n, const float* taps, int up, int down, int half,
                                 float* out, hipStream_t stream) {
  CSTS_REQUIRE(wav && taps && out, "bad args");
  CSTS_REQUIRE(in_kind == CSTS_WAV_F32 || in_kind == CSTS_WAV_I16, "in_kind must be CSTS_WAV_F32 or CSTS_WAV_I16");
  CSTS_REQUIRE(B > 0 && B <= 65535 && C > 0 && C <= 64 && n > 0 && n <= CSTS_RESAMPLE_MAX_N, "bad sizes (B <= 65535, C <= 64, n <= 2^40)");
  CSTS_REQUIRE(up > 0 && down > 0 && up <= CSTS_RESAMPLE_MAX_RATIO && down <= CSTS_RESAMPLE_MAX_RATIO && half > 0 &&
                   half <= CSTS_RESAMPLE_MAX_RATIO, "bad ratio (1 <= up, down, half <= 2^20)");
  const int64_t P = phase_taps(up, half), pstride = P | 1, cap = span_cap(up, down, half);
  const int64_t floats = up * pstride + skewed(cap);
  CSTS_REQUIRE(floats <= CSTS_RESAMPLE_MAX_LDS_FLOATS, "the filter table and one run's input span do not fit the kernel's LDS");
  const int64_t n_out = csts_resample_len(n, up, down);
  const int64_t nruns = cdiv(n_out, RUN);
  const dim3 grid((unsigned)std::min<int64_t>(nruns, 2048), B);
  const size_t lds = (size_t)floats * sizeof(float);
  if (in_kind == CSTS_WAV_F32)
    hipLaunchKernelGGL((resample_kernel<float, false>), grid, dim3(256), lds, stream, static_cast<const float*>(wav), C, n, (int64_t)0, taps, up,
                       down, half, (int)P, (int)pstride, (int)cap, (int64_t)0, n_out, nruns, out);
  else
    hipLaunchKernelGGL((resample_kernel<int16_t, false>), grid, dim3(256), lds, stream, static_cast<const int16_t*>(wav), C, n, (int64_t)0, taps,
                       up, down, half, (int)P, (int)pstride, (int)cap, (int64_t)0, n_out, nruns, out);
  CSTS_LAUNCH_CHECK();
  return 0;
}

// ---- the same rule on a stream that arrives in pieces (inputs.StreamResampler) -------------------------------------------------
namespace {
inline bool ratio_ok(int up, int down, int half) {
  return up > 0 && down > 0 && half > 0 && up <= CSTS_RESAMPLE_MAX_RATIO && down <= CSTS_RESAMPLE_MAX_RATIO && half <= CSTS_RESAMPLE_MAX_RATIO;
}
inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }                           // b > 0
}  // namespace

// Output m reads the inputs up to floor((m down + half) / up): it is final once that sample is in, or once the stream has ended.
extern "C" int64_t csts_resample_ready(int64_t n_in, int up, int down, int half, int closed) {
  if (n_in < 0 || n_in > CSTS_RESAMPLE_MAX_N || !ratio_ok(up, down, half)) return -1;
  if (closed) return (n_in * up + down - 1) / down;
  return std::max<int64_t>(0, floor_div(n_in * up - half - 1, down) + 1);
}

extern "C" int64_t csts_resample_first_input(int64_t m, int up, int down, int half) {
  if (m < 0 || !ratio_ok(up, down, half) || m > ((int64_t)1 << 61) / down) return -1;                 // m * down stays in 64 bits
  return std::max<int64_t>(0, -floor_div(-(m * down - half), up));
}

extern "C" int csts_resample_stream(const void* buf, int in_kind, int C, int64_t len, int64_t x_base, int64_t n_total, const float* taps,
                                    int up, int down, int half, int64_t m0, int64_t m1, float* out, hipStream_t stream) {
  CSTS_REQUIRE(in_kind == CSTS_WAV_F32 || in_kind == CSTS_WAV_I16, "in_kind must be CSTS_WAV_F32 or CSTS_WAV_I16");
  CSTS_REQUIRE(ratio_ok(up, down, half), "bad ratio (1 <= up, down, half <= 2^20)");
  CSTS_REQUIRE(m0 >= 0 && m0 <= m1, "bad output range (0 <= m0 <= m1)");
  if (m0 == m1) return 0;
  CSTS_REQUIRE(buf && taps && out, "bad args");
  CSTS_REQUIRE(C > 0 && C <= 64 && len > 0 && x_base >= 0 && len <= CSTS_RESAMPLE_MAX_N && x_base <= CSTS_RESAMPLE_MAX_N - len,
               "bad sizes (C <= 64, 1 <= len, x_base + len <= 2^40)");
  const int64_t P = phase_taps(up, half), pstride = P | 1, cap = span_cap(up, down, half);
  const int64_t floats = up * pstride + skewed(cap);
  CSTS_REQUIRE(floats <= CSTS_RESAMPLE_MAX_LDS_FLOATS, "the filter table and one run's input span do not fit the kernel's LDS");
  const int64_t have = x_base + len;
  if (n_total < 0) {
    CSTS_REQUIRE(m1 <= csts_resample_ready(have, up, down, half, 0), "an output of an open stream reads a sample that is not in the buffer yet");
  } else {
    CSTS_REQUIRE(have == n_total, "the buffer of a closed stream ends at its last sample (x_base + len == n_total)");
    CSTS_REQUIRE(m1 <= csts_resample_ready(n_total, up, down, half, 1), "m1 is past ceil(n_total * up / down)");
  }
  CSTS_REQUIRE(csts_resample_first_input(m0, up, down, half) >= x_base, "the first input of output m0 lies before x_base");
  const int64_t nruns = cdiv(m1 - m0, RUN);
  const dim3 grid((unsigned)std::min<int64_t>(nruns, 2048), 1);
  const size_t lds = (size_t)floats * sizeof(float);
  if (in_kind == CSTS_WAV_F32)
    hipLaunchKernelGGL((resample_kernel<float, true>), grid, dim3(256), lds, stream, static_cast<const float*>(buf), C, len, x_base, taps, up,
                       down, half, (int)P, (int)pstride, (int)cap, m0, m1, nruns, out);
  else
    hipLaunchKernelGGL((resample_kernel<int16_t, true>), grid, dim3(256), lds, stream, static_cast<const int16_t*>(buf), C, len, x_base, taps,
                       up, down, half, (int)P, (int)pstride, (int)cap, m0, m1, nruns, out);
  CSTS_LAUNCH_CHECK();
  return 0;
}
