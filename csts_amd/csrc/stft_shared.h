// The log-power STFT column input.hip (a whole waveform) and stream.hip (an endless signal, columns into a ring) share: one
// workgroup of 256 threads computes column f -- the window's samples times the periodic Hann window and the twiddle table in
// LDS, one thread per bin, a 240-tap direct DFT.  Both kernels call this one body, so a column has the same bits in either.
#pragma once
#include "common.h"

namespace {

// dynamic LDS floats of one column: [win] windowed samples, [n_fft] cos, [n_fft] sin
__host__ __device__ __forceinline__ int stft_lds_floats(int n_fft, int win) { return win + 2 * n_fft; }

// first waveform sample under the window of column f (center=True; librosa.util.pad_center of the window inside n_fft)
__host__ __device__ __forceinline__ int64_t stft_first_sample(int64_t f, int n_fft, int hop, int win) {
  return f * hop + (n_fft - win) / 2 - n_fft / 2;
}

// Column f of log(|STFT|^2 + eps).  inside(s): sample s exists (any other sample is zero); get(s): its value, called only where
// inside(s).  Bin `bin` goes to dst[bin * bin_stride].  Every thread of the 256-thread workgroup calls it with the same arguments
// (it holds a barrier); sm: stft_lds_floats(n_fft, win) floats.
template <class Inside, class Get>
__device__ __forceinline__ void stft_logpower_column(float* sm, int64_t f, int n_fft, int hop, int win, float eps, Inside inside,
                                                     Get get, float* __restrict__ dst, int64_t bin_stride) {
  float* xs = sm;
  float* ct = sm + win;
  float* st = ct + n_fft;
  const int tid = threadIdx.x;
  const int lpad = (n_fft - win) / 2;
  const int64_t s0 = stft_first_sample(f, n_fft, hop, win);
  for (int k = tid; k < win; k += 256) {
    const int64_t s = s0 + k;
    const float w = 0.5f - 0.5f * cospif(2.0f * (float)k / (float)win);     // scipy hann, fftbins=True
    xs[k] = inside(s) ? get(s) * w : 0.f;
  }
  for (int m = tid; m < n_fft; m += 256) {
    float sv, cv;
    sincospif(2.0f * (float)m / (float)n_fft, &sv, &cv);
    ct[m] = cv; st[m] = sv;
  }
  __syncthreads();
  const int nbins = n_fft / 2 + 1;
  for (int bin = tid; bin < nbins; bin += 256) {
    float re = 0.f, im = 0.f;
    int idx = (int)(((int64_t)bin * lpad) % n_fft);            // phase index (bin * j) mod n_fft, j = lpad + k
    for (int k = 0; k < win; ++k) {
      re += xs[k] * ct[idx];
      im -= xs[k] * st[idx];
      idx += bin;
      if (idx >= n_fft) idx -= n_fft;
    }
    dst[(int64_t)bin * bin_stride] = logf(re * re + im * im + eps);
  }
}

}  // namespace
