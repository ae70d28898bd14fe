// The small streaming kernels of the library and their extern "C" entries (profiling kind misc, no workspace).  Each walks its
// operand once with 256-thread blocks, sums in double where it reduces, and is HBM- or launch-bound.
//   ttr_norm            out[b] = ||x[b]||_2; one block per item  (torch.norm: tensor.py:2039-2051, round.py:80)
//   ttr_scale_cols      out[b][:, j] = in[b][:, j] * s[b][j], or / s[b][j] (0 where |s| < tiny); grid (<= 2048 strides, items)
//                       (left * sigma: round.py:169-172)
//   ttr_mask_cols       x[b][:, j] = 0 for j >= keep[b] (keep[b] < 0 counts as 0); grid (<= 1024 strides, items)
//                       (left = vectors[..., :rank] with the rank on the device: round.py:160-161)
//   ttr_spectrum_flat   flat[b] = 1 when item b's spectrum lets it skip the second Gram pass; one thread per item
//   ttr_carry_rows32    flag[b] = 1 when rows 32.. of the 64-row R[b] are negligible; one block per item
//                       (the packing test of ttr_qr.hip for the last core of a sweep, which no push follows)
//   ttr_pow2_normalize  out[b] = x[b] * 2^-e with e the binary exponent of ||x[b]||_2 (exact); one block per item
//   ttr_scale_batch     out[b] = x[b] * scale[b] * 2^(sign * expo[b]); grid (<= 1024 strides, items)
// Every index is bounded by the validated host arguments (count, rows x cols, batch).  A batch beyond the 65535 limit of
// gridDim.y runs in slices (ttr_mask_cols: rejected).  sumsq_partial_kernel, the first stage of a two-stage norm of one long
// vector, is launched by no entry.
#include "detail/ttr_internal.h"

namespace ttr {

template <typename T>
__global__ __launch_bounds__(kThreads) void norm_kernel(const T* __restrict__ x, int64_t count, int64_t stride_x,
                                                        T* __restrict__ out) {
  __shared__ double red[kThreads / kWave];
  const int64_t b = blockIdx.x;
  const T* __restrict__ xb = x + b * stride_x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += kThreads) {
    const double v = (double)xb[i];
    acc += v * v;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int w = 0; w < kThreads / kWave; ++w) s += red[w];
    out[b] = (T)sqrt(s);
  }
}

// Large single vectors: two-stage (partials per workgroup, then a finishing workgroup).
template <typename T>
__global__ __launch_bounds__(kThreads) void sumsq_partial_kernel(const T* __restrict__ x, int64_t count,
                                                                 double* __restrict__ part) {
  __shared__ double red[kThreads / kWave];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kThreads) {
    const double v = (double)x[i];
    acc += v * v;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int w = 0; w < kThreads / kWave; ++w) s += red[w];
    part[blockIdx.x] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void scale_cols_kernel(int64_t rows, int64_t cols, const T* __restrict__ in,
                                                              int64_t ldi, int64_t stride_in, const T* __restrict__ s,
                                                              int64_t stride_s, int mode, T* __restrict__ out,
                                                              int64_t ldo, int64_t stride_out) {
  const int64_t b = blockIdx.y;
  const int64_t total = rows * cols;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
    const int64_t i = idx / cols, j = idx % cols;
    const T v = in[b * stride_in + i * ldi + j];
    const T sj = s[b * stride_s + j];
    T r;
    if (mode == TTR_SCALE_MUL) r = v * sj;
    else r = (fabs((double)sj) < (double)Num<T>::tiny()) ? T(0) : v / sj;
    out[b * stride_out + i * ldo + j] = r;
  }
}

// x[b][:, j] <- 0 for j >= keep[b] (in place): the device-side truncation of an eps-mode sweep that computes every bond at
// its rank CAP and never reads the selected rank back (keep = the eigensolver's info[b]; 0 = zero guard: everything goes)
template <typename T>
__global__ __launch_bounds__(kThreads) void mask_cols_kernel(int64_t rows, int64_t cols, T* __restrict__ x, int64_t ldx,
                                                             int64_t stride_x, const int32_t* __restrict__ keep) {
  const int64_t b = blockIdx.y;
  const int64_t k = keep[b] < 0 ? 0 : keep[b];  // (a negative count keeps nothing: j = k + idx % w must not start before the row)
  if (k >= cols) return;
  const int64_t w = cols - k, total = rows * w;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
    const int64_t i = idx / w, j = k + idx % w;
    x[b * stride_x + i * ldx + j] = T(0);
  }
}

// flat[b] = 1 when the `keep` largest singular values of item b (sigma sorted decreasing) lie within a factor 1 / thr of
// each other: sigma[keep - 1] >= thr * sigma[0] > 0
template <typename T>
__global__ void spectrum_flat_kernel(int64_t batch, int n, int keep, T thr, const T* __restrict__ sigma, int64_t stride_sigma,
                                     int use_delta, double delta2, const double* __restrict__ delta2_dev, int32_t* __restrict__ flat,
                                     int noise_c, const int32_t* __restrict__ rows32, int n_full) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  // `rows32` items (the carry of a packed bond: rows 32.. are exactly zero, ttr_rowgram): sigma[32..] are STRUCTURAL zeros -- exact
  // in pass 1 and in pass 2 alike -- so what the rule decides about them is certain and only the 32 computed values carry pass 1's
  // error.  The rule sees them at the noise floor c eps sigma_0 (TTR_KNOB_RANK_NOISE_FLOOR, rank_rule in ttr_common.h; 0 when the
  // floor is off): a fixed, known tail energy nstruct (c eps sigma_0)^2 that enters the sums below without an error bar.
  // (Round 6: with the floor on by default the 32 zeros used to be treated like computed values "within E of delta^2" -- no
  // rows32 item of an fp32 eps-mode sweep took the one-pass shortcut any more, 1.63 -> 1.85 ms for round_tt(eps=1e-4) of one 64^8 train.)
  const int nstruct = (rows32 && rows32[b] != 0 && n > 32) ? n - 32 : 0;
  n -= nstruct;                      // computed values: sigma[0 .. n)
  if (keep > n + nstruct) keep = n + nstruct;
  const T* __restrict__ sgr = sigma + b * stride_sigma;
  const T s0 = sgr[0];
  // (the rank rule's view of the spectrum: rank_rule in ttr_common.h -- with TTR_KNOB_RANK_NOISE_FLOOR nothing lies below c eps sigma_0)
  const T nfl = noise_c > 0 ? T(noise_c) * Num<T>::eps() * s0 : T(0);
  auto sg = [&](int k) { const T v = k < n ? sgr[k] : T(0); return v < nfl ? nfl : v; };   // (k >= n: a structural zero at the floor)
  int kp = keep;
  bool ok = s0 > T(0);
  const double d2 = use_delta ? (delta2_dev ? *delta2_dev : delta2) : 0.0;
  if (ok && d2 > 0.0) {
    // eps mode: the rank comes from the tail energies of pass 1's sigma, which carry an absolute error of up to E = 64 n eps sigma_1^2
    // (n values, each c eps sigma_1^2 off); the item only qualifies when the rule's decision is the same for every spectrum within E
    // of this one -- tail(r) <= delta^2 - E and tail(r - 1) > delta^2 + E at the selected rank r (rank cap binding: only the latter)
    const int nt = n + nstruct;
    const double E = 64.0 * n_full * (double)Num<T>::eps() * (double)s0 * (double)s0;
    double acc = 0.0, tail_r = 0.0;
    int tail = 0;
    for (int k = nt - 1; k >= 0; --k) {
      acc += (double)sg(k) * (double)sg(k);
      if (acc <= d2) { tail = nt - k; tail_r = acc; } else break;
    }
    int r = nt - tail;
    if (r < 1) r = 1;
    if (r > keep) {  // the cap decides as long as the rule cannot cut the keep-th value: tail(keep - 1) > delta^2 + E
      double tc = 0.0;
      for (int k = nt - 1; k >= keep - 1; --k) tc += (double)sg(k) * (double)sg(k);
      // (a keep-th value that is itself structural is known exactly: no error bar)
      ok = keep - 1 >= n ? tc > d2 : tc > d2 + E;
      kp = keep;
    } else {
      const int rr = nt - tail;  // the rule's rank before the ">= 1" clamp
      // what is cut stays cut: nothing computed is cut (only structural zeros: certain), or the computed tail keeps its distance
      const bool cut_safe = tail <= nstruct || tail_r <= d2 - E;
      bool keep_safe = true;                                 // the last kept value cannot be cut as well (rr = 0: rank 1 either way)
      if (rr >= 1) keep_safe = rr - 1 >= n ? (tail_r + (double)sg(rr - 1) * (double)sg(rr - 1) > d2)
                                           : (tail_r + (double)sg(rr - 1) * (double)sg(rr - 1) > d2 + E);
      ok = cut_safe && keep_safe;
      kp = r;
    }
  }
  flat[b] = (ok && sg(kp - 1) >= thr * s0) ? 1 : 0;
}

// flag[b] = 1 when rows 32.. of the 64-row matrix R[b] hold at most (c eps)^2 of its squared Frobenius norm -- the packing test of
// the fused push + factor kernel (ttr_qr.hip: `packed`), for the LAST core of a sweep, which no push follows
template <typename T>
__global__ __launch_bounds__(kThreads) void carry_rows32_kernel(int64_t cols, const T* __restrict__ R, int64_t ldr, int64_t strideR,
                                                                double ce2, int32_t* __restrict__ flag) {
  __shared__ double red[kThreads / kWave];
  const int64_t b = blockIdx.x;
  const T* __restrict__ Rb = R + b * strideR;
  double all = 0.0, low = 0.0;
  for (int64_t idx = threadIdx.x; idx < 64 * cols; idx += kThreads) {
    const int64_t i = idx / cols, j = idx - i * cols;
    const double v = (double)Rb[i * ldr + j];
    all += v * v;
    if (i >= 32) low += v * v;
  }
  all = block_sum(all, red);
  low = block_sum(low, red);
  if (threadIdx.x == 0) flag[b] = (ce2 > 0.0 && low <= ce2 * all) ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void pow2_normalize_kernel(const T* __restrict__ x, int64_t count, int64_t stride_x,
                                                                  T* __restrict__ out, int64_t stride_out,
                                                                  int32_t* __restrict__ e_out, int32_t* __restrict__ expo_acc) {
  __shared__ double red[kThreads / kWave];
  const int64_t b = blockIdx.x;
  const T* __restrict__ xb = x + b * stride_x;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += kThreads) {
    const double v = (double)xb[i];
    acc += v * v;
  }
  const double nrm = sqrt(block_sum(acc, red));
  int e = 0;
  if (nrm > 0.0 && nrm < 1e300) (void)frexp(nrm, &e);
  if (out) {
    T* __restrict__ ob = out + b * stride_out;
    for (int64_t i = threadIdx.x; i < count; i += kThreads) ob[i] = (T)ldexp((double)xb[i], -e);  // exact
  }
  if (threadIdx.x == 0) {
    if (e_out) e_out[b] = e;
    if (expo_acc) expo_acc[b] += e;
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void scale_batch_kernel(const T* __restrict__ x, int64_t count, int64_t stride_x,
                                                               const T* __restrict__ scale, int64_t stride_scale,
                                                               const int32_t* __restrict__ expo, int expo_sign,
                                                               T* __restrict__ out, int64_t stride_out) {
  const int64_t b = blockIdx.y;
  const T sc = scale ? scale[b * stride_scale] : T(1);
  const int e = expo ? expo_sign * expo[b] : 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kThreads) {
    T v = x[b * stride_x + i] * sc;
    if (e != 0) v = (T)ldexp((double)v, e);
    out[b * stride_out + i] = v;
  }
}

}  // namespace ttr

using namespace ttr;

extern "C" {

int ttr_norm(int dtype, int64_t count, int64_t batch, const void* x, int64_t stride_x, void* out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_norm: bad dtype %d", dtype);
  TTR_REQUIRE(count >= 0 && batch >= 0, TTR_E_INVALID, "ttr_norm: negative size");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(x && out, TTR_E_INVALID, "ttr_norm: null pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(norm_kernel<T>, dim3((unsigned)batch), dim3(kThreads), 0, s, (const T*)x, count, stride_x, (T*)out);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_scale_cols(int dtype, int64_t rows, int64_t cols, int64_t batch, const void* in, int64_t ldi,
                   int64_t stride_in, const void* sc, int64_t stride_s, int mode, void* out, int64_t ldo,
                   int64_t stride_out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_scale_cols: bad dtype %d", dtype);
  TTR_REQUIRE(mode == TTR_SCALE_MUL || mode == TTR_SCALE_DIV, TTR_E_INVALID, "ttr_scale_cols: bad mode");
  if (rows <= 0 || cols <= 0 || batch <= 0) return TTR_OK;
  TTR_REQUIRE(in && sc && out, TTR_E_INVALID, "ttr_scale_cols: null pointer");
  if (batch > 65535) {  // the batch is a grid dimension: slices
    const int64_t elem = elem_size(dtype);
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
      const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
      const int rc = ttr_scale_cols(dtype, rows, cols, nb, (const char*)in + b0 * stride_in * elem, ldi, stride_in,
                                    (const char*)sc + b0 * stride_s * elem, stride_s, mode, (char*)out + b0 * stride_out * elem, ldo,
                                    stride_out, stream);
      if (rc != TTR_OK) return rc;
    }
    return TTR_OK;
  }
  hipStream_t s = (hipStream_t)stream;
  int64_t gx = ceil_div(rows * cols, kThreads);
  if (gx > 2048) gx = 2048;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(scale_cols_kernel<T>, dim3((unsigned)gx, (unsigned)batch), dim3(kThreads), 0, s, rows, cols, (const T*)in, ldi,
                       stride_in, (const T*)sc, stride_s, mode, (T*)out, ldo, stride_out);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_mask_cols(int dtype, int64_t rows, int64_t cols, int64_t batch, void* x, int64_t ldx, int64_t stride_x,
                  const int32_t* keep, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_mask_cols: bad dtype %d", dtype);
  if (rows <= 0 || cols <= 0 || batch <= 0) return TTR_OK;
  TTR_REQUIRE(x && keep, TTR_E_INVALID, "ttr_mask_cols: null pointer");
  TTR_REQUIRE(batch <= 65535, TTR_E_UNSUPPORTED, "ttr_mask_cols: batch %lld > 65535", (long long)batch);
  hipStream_t s = (hipStream_t)stream;
  int64_t gx = ceil_div(rows * cols, kThreads);
  if (gx > 1024) gx = 1024;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mask_cols_kernel<T>, dim3((unsigned)gx, (unsigned)batch), dim3(kThreads), 0, s, rows, cols, (T*)x, ldx, stride_x,
                       keep);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_carry_rows32(int dtype, int64_t cols, int64_t batch, const void* R, int64_t ldr, int64_t strideR, int32_t* flag,
                     void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_carry_rows32: bad dtype %d", dtype);
  TTR_REQUIRE(cols >= 1 && batch >= 0 && ldr >= cols, TTR_E_INVALID, "ttr_carry_rows32: bad shape");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(R && flag, TTR_E_INVALID, "ttr_carry_rows32: null pointer");
  hipStream_t s = (hipStream_t)stream;
  // the thresholds of the packing test (TTR_KNOB_QR_RANK_SKIP, TTR_KNOB_QR_PACK = 0: never)
  const double ce = (g_qr_pack ? (double)g_rank_skip_c : 0.0) * (dtype == TTR_F32 ? 1.1920929e-07 : 2.220446049250313e-16);
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(carry_rows32_kernel<T>, dim3((unsigned)batch), dim3(kThreads), 0, s, cols, (const T*)R, ldr, strideR, ce * ce,
                       flag);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_spectrum_flat(int dtype, int64_t n, int64_t batch, const void* sigma, int64_t stride_sigma, int64_t keep, double thr,
                      int use_delta, double delta2, const double* delta2_dev, int32_t* flat, const int32_t* rows32,
                      void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_spectrum_flat: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 1 && keep >= 1 && keep <= n && batch >= 0 && thr > 0.0 && thr <= 1.0 && delta2 >= 0.0, TTR_E_INVALID,
              "ttr_spectrum_flat: bad arguments");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(sigma && flat, TTR_E_INVALID, "ttr_spectrum_flat: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const unsigned gx = (unsigned)ceil_div(batch, kThreads);
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(spectrum_flat_kernel<T>, dim3(gx), dim3(kThreads), 0, s, batch, (int)n, (int)keep, (T)thr, (const T*)sigma,
                       stride_sigma, use_delta, delta2, delta2_dev, flat, g_rank_noise_c, rows32, (int)n);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_pow2_normalize(int dtype, int64_t count, int64_t batch, const void* x, int64_t stride_x, void* out,
                       int64_t stride_out, int32_t* e_out, int32_t* expo_acc, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_pow2_normalize: bad dtype %d", dtype);
  TTR_REQUIRE(count >= 0 && batch >= 0, TTR_E_INVALID, "ttr_pow2_normalize: negative size");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(x && (out || e_out), TTR_E_INVALID, "ttr_pow2_normalize: null pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(TTR_PROF_MISC, s);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(pow2_normalize_kernel<T>, dim3((unsigned)batch), dim3(kThreads), 0, s, (const T*)x, count, stride_x, (T*)out,
                       stride_out, e_out, expo_acc);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

int ttr_scale_batch(int dtype, int64_t count, int64_t batch, const void* x, int64_t stride_x, const void* scale,
                    int64_t stride_scale, const int32_t* expo, int expo_sign, void* out, int64_t stride_out,
                    void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_scale_batch: bad dtype %d", dtype);
  TTR_REQUIRE(count >= 0 && batch >= 0, TTR_E_INVALID, "ttr_scale_batch: negative size");
  if (batch == 0 || count == 0) return TTR_OK;
  TTR_REQUIRE(x && out, TTR_E_INVALID, "ttr_scale_batch: null pointer");
  hipStream_t s = (hipStream_t)stream;
  int64_t gx = ceil_div(count, kThreads * 4);
  if (gx > 1024) gx = 1024;
  if (gx < 1) gx = 1;
  ProfScope prof(TTR_PROF_MISC, s);
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {  // gridDim.y limit
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    const int64_t so = elem_size(dtype);
    const char* xs = (const char*)x + b0 * stride_x * so;
    char* os = (char*)out + b0 * stride_out * so;
    const char* ss = scale ? (const char*)scale + b0 * stride_scale * so : nullptr;
    const int32_t* es = expo ? expo + b0 : nullptr;
    by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(scale_batch_kernel<T>, dim3((unsigned)gx, (unsigned)nb), dim3(kThreads), 0, s, (const T*)xs, count, stride_x,
                         (const T*)ss, stride_scale, es, expo_sign, (T*)os, stride_out);
    });
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // extern "C"
