// extern "C" surface of libttround_hip.so for the kernels of ttr_gemm / ttr_qr / ttr_eigh / ttr_bjacobi / ttr_sweep / ttr_cp /
// ttr_eigsel .hip (thin validating wrappers around their dispatchers, detail/ttr_internal.h), error reporting, the knob
// setter, and the per-kernel HIP-event profiler and executed-work census used by bench.py.  The other entries live next to
// their kernels: ttr_vec.hip, ttr_orth.hip, ttr_roundtt.hip and the files of the later features.
#include <stdarg.h>

#include <mutex>
#include <vector>

#include "detail/ttr_internal.h"

namespace ttr {

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
  return TTR_E_HIP;
}

// ------------------------------------------------------------------ profiler
struct ProfRec {
  int kind;
  hipEvent_t start, stop;
};
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof_recs;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;

ProfScope::ProfScope(int kind_, hipStream_t s) : kind(kind_), stream(s), slot(nullptr) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  ProfRec r;
  r.kind = kind;
  if (!g_prof_pool.empty()) {
    r.start = g_prof_pool.back().first;
    r.stop = g_prof_pool.back().second;
    g_prof_pool.pop_back();
  } else {
    if (hipEventCreate(&r.start) != hipSuccess || hipEventCreate(&r.stop) != hipSuccess) return;
  }
  (void)hipEventRecord(r.start, stream);
  g_prof_recs.push_back(r);
  slot = (void*)(uintptr_t)g_prof_recs.size();  // index + 1
}

ProfScope::~ProfScope() {
  if (!slot) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  const size_t idx = (size_t)(uintptr_t)slot - 1;
  if (idx < g_prof_recs.size()) (void)hipEventRecord(g_prof_recs[idx].stop, stream);
}

// ------------------------------------------------------------------ executed-work census
static int g_prof_level = 0;          // 0 off, 1 = times, 2 = times + executed-work census
static double* g_work_dev = nullptr;  // [2 * TTR_PROF_NKINDS]: flops per kind, then bytes per kind

bool work_census_on() { return g_prof_level >= 2 && g_work_dev != nullptr; }
double* work_census_dev() { return work_census_on() ? g_work_dev : nullptr; }

__global__ void work_items_kernel(const int32_t* __restrict__ f1, const int32_t* __restrict__ f2, int64_t batch, double fl0, double fl1,
                                  double fl2, double fl3, double by0, double by1, double by2, double by3, double* __restrict__ out_fl,
                                  double* __restrict__ out_by) {
  __shared__ double red[2 * kThreads / kWave];
  double a = 0.0, c = 0.0;
  for (int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x; b < batch; b += (int64_t)gridDim.x * kThreads) {
    const int k = ((f1 && f1[b] != 0) ? 1 : 0) + ((f2 && f2[b] != 0) ? 2 : 0);
    a += k == 0 ? fl0 : k == 1 ? fl1 : k == 2 ? fl2 : fl3;
    c += k == 0 ? by0 : k == 1 ? by1 : k == 2 ? by2 : by3;
  }
  a = wave_sum(a); c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[kThreads / kWave + (threadIdx.x >> 6)] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / kWave; ++w) { a += red[w]; c += red[kThreads / kWave + w]; }
    atomicAdd(out_fl, a);
    atomicAdd(out_by, c);
  }
}

void work_items(int kind, const int32_t* f1, const int32_t* f2, int64_t batch, const double fl[4], const double by[4], hipStream_t s) {
  if (!work_census_on() || batch <= 0) return;
  int64_t gx = ceil_div(batch, kThreads);
  if (gx > 256) gx = 256;
  hipLaunchKernelGGL(work_items_kernel, dim3((unsigned)gx), dim3(kThreads), 0, s, f1, f2, batch, fl[0], fl[1], fl[2], fl[3], by[0], by[1],
                     by[2], by[3], g_work_dev + kind, g_work_dev + TTR_PROF_NKINDS + kind);
}

template <typename T>
__global__ void work_qr_taus_kernel(const T* __restrict__ tau, int64_t nblk, int64_t nb_per_item, int NP, int64_t m, int64_t rpb, int n,
                                    int kc, int reads_input, const int32_t* __restrict__ live_half, double* __restrict__ out_fl,
                                    double* __restrict__ out_by) {
  __shared__ double red[2 * kThreads / kWave];
  double a = 0.0, by = 0.0;
  const double s = (double)sizeof(T);
  for (int64_t blk = (int64_t)blockIdx.x * kThreads + threadIdx.x; blk < nblk; blk += (int64_t)gridDim.x * kThreads) {
    const T* __restrict__ t = tau + blk * NP;
    int q = 0;
    for (int pnl = 0; pnl < NP / 16; ++pnl) {
      bool live = false;
      for (int j = 0; j < 16; ++j) live = live || (t[16 * pnl + j] != T(0));
      q += live ? 1 : 0;
    }
    const int64_t b = blk % nb_per_item;
    double r = (double)(m - b * rpb < rpb ? m - b * rpb : rpb);
    if (r < 0) r = 0;
    const double rl = (live_half && live_half[blk / nb_per_item] == 3) ? 0.5 * r : r;   // rows the launch computes on (QrLevel::live_half)
    double c = 16.0 * q;
    if (c > n) c = n;
    if (kc > 0) {
      a += 4.0 * r * c * kc;
      by += s * (r * c + (q > 0 ? r * kc : 0.0));                       // live reflectors read, the block's output rows written
    } else {
      a += 2.0 * rl * c * c - 2.0 * c * c * c / 3.0 + 4.0 * rl * c * (n - c);
      by += s * (r * c + (q > 0 ? (double)n * n : 0.0) + (reads_input ? r * n : 0.0));   // reflectors + R written (+ the block read)
    }
  }
  a = wave_sum(a); by = wave_sum(by);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[kThreads / kWave + (threadIdx.x >> 6)] = by; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / kWave; ++w) { a += red[w]; by += red[kThreads / kWave + w]; }
    atomicAdd(out_fl, a);
    atomicAdd(out_by, by);
  }
}

void work_qr_taus(int kind, const void* tau, bool f64, int64_t nblk, int64_t nb_per_item, int NP, int64_t m, int64_t rpb, int n,
                  int kc, bool reads_input, hipStream_t s, const int32_t* live_half) {
  if (!work_census_on() || nblk <= 0) return;
  int64_t gx = ceil_div(nblk, kThreads);
  if (gx > 512) gx = 512;
  double* fl = g_work_dev + kind;
  double* by = g_work_dev + TTR_PROF_NKINDS + kind;
  if (f64)
    hipLaunchKernelGGL(work_qr_taus_kernel<double>, dim3((unsigned)gx), dim3(kThreads), 0, s, (const double*)tau, nblk, nb_per_item, NP, m,
                       rpb, n, kc, reads_input ? 1 : 0, live_half, fl, by);
  else
    hipLaunchKernelGGL(work_qr_taus_kernel<float>, dim3((unsigned)gx), dim3(kThreads), 0, s, (const float*)tau, nblk, nb_per_item, NP, m,
                       rpb, n, kc, reads_input ? 1 : 0, live_half, fl, by);
}

}  // namespace ttr

using namespace ttr;

extern "C" {

int ttr_version(void) { return TTR_ABI_VERSION; }

const char* ttr_last_error(void) { return g_err.c_str(); }

int ttr_qr_max_cols(int dtype) { return qr_max_cols(dtype); }
int ttr_eigh_max_n_lds(int dtype) { return eigh_max_n_lds(dtype); }
int ttr_eigh_max_n(int dtype) { return eigh_max_n(dtype); }

int64_t ttr_gemm_workspace_bytes(int dtype, int64_t M, int64_t N, int64_t K, int64_t batch) {
  return gemm_workspace_bytes(dtype, M, N, K, batch);
}

int ttr_gemm(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
             int64_t strideA, const void* B, int64_t ldb, int64_t strideB, void* C, int64_t ldc, int64_t strideC,
             const void* rowscale, int64_t stride_rs, int rowscale_mode, const void* colscale, int64_t stride_cs,
             int colscale_mode, int64_t batch, void* workspace, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_gemm: bad dtype %d", dtype);
  TTR_REQUIRE(M >= 0 && N >= 0 && K >= 0 && batch >= 0, TTR_E_INVALID, "ttr_gemm: negative dimension");
  if (M == 0 || N == 0 || batch == 0) return TTR_OK;
  TTR_REQUIRE(K >= 1, TTR_E_INVALID, "ttr_gemm: K must be >= 1");
  TTR_REQUIRE(A && B && C, TTR_E_INVALID, "ttr_gemm: null operand");
  return gemm_dispatch(dtype, transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, rowscale,
                       stride_rs, rowscale_mode, colscale, stride_cs, colscale_mode, batch, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int ttr_gemm_axpby(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                   int64_t strideA, const void* B, int64_t ldb, int64_t strideB, void* C, int64_t ldc, int64_t strideC,
                   double alpha, double beta, int64_t batch, void* workspace, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_gemm_axpby: bad dtype %d", dtype);
  TTR_REQUIRE(M >= 0 && N >= 0 && K >= 0 && batch >= 0, TTR_E_INVALID, "ttr_gemm_axpby: negative dimension");
  if (M == 0 || N == 0 || batch == 0) return TTR_OK;
  TTR_REQUIRE(K >= 1, TTR_E_INVALID, "ttr_gemm_axpby: K must be >= 1");
  TTR_REQUIRE(A && B && C, TTR_E_INVALID, "ttr_gemm_axpby: null operand");
  return gemm_dispatch(dtype, transA, transB, M, N, K, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, nullptr, 0,
                       TTR_SCALE_NONE, nullptr, 0, TTR_SCALE_NONE, batch, workspace, workspace_bytes,
                       (hipStream_t)stream, 1, alpha, beta);
}

int64_t ttr_qr_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t batch) {
  return qr_workspace_bytes(dtype, m, n, batch);
}

int ttr_qr_factor(int dtype, int64_t m, int64_t n, int64_t batch, const void* A, int64_t lda, int64_t strideA, void* R,
                  int64_t ldr, int64_t strideR, void* workspace, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_qr_factor: bad dtype %d", dtype);
  TTR_REQUIRE(m >= 1 && n >= 1 && batch >= 0, TTR_E_INVALID, "ttr_qr_factor: bad shape %lld x %lld", (long long)m,
              (long long)n);
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(A && R && workspace, TTR_E_INVALID, "ttr_qr_factor: null pointer");
  return qr_factor_dispatch(dtype, m, n, batch, A, lda, strideA, R, ldr, strideR, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

int ttr_qr_factor_expo(int dtype, int64_t m, int64_t n, int64_t batch, const void* A, int64_t lda, int64_t strideA, void* R,
                       int64_t ldr, int64_t strideR, void* workspace, int64_t workspace_bytes, int32_t* expo_acc, void* stream) {
  TTR_REQUIRE(dtype == TTR_F32, TTR_E_UNSUPPORTED, "ttr_qr_factor_expo: fp32 only (dtype %d)", dtype);
  TTR_REQUIRE(m >= 1 && n >= 1 && batch >= 0, TTR_E_INVALID, "ttr_qr_factor_expo: bad shape %lld x %lld", (long long)m,
              (long long)n);
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(A && R && workspace && expo_acc, TTR_E_INVALID, "ttr_qr_factor_expo: null pointer");
  return qr_factor_dispatch(dtype, m, n, batch, A, lda, strideA, R, ldr, strideR, workspace, workspace_bytes,
                            (hipStream_t)stream, 1, expo_acc);
}

int ttr_qr_apply(int dtype, int64_t m, int64_t n, int64_t batch, void* workspace, int64_t workspace_bytes,
                 const void* C, int64_t ldc, int64_t strideC, int64_t kcols, void* Out, int64_t ldo, int64_t strideO,
                 void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_qr_apply: bad dtype %d", dtype);
  TTR_REQUIRE(m >= 1 && n >= 1 && batch >= 0 && kcols >= 1, TTR_E_INVALID, "ttr_qr_apply: bad shape");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(Out && workspace, TTR_E_INVALID, "ttr_qr_apply: null pointer");
  TTR_REQUIRE(kcols <= (m < n ? m : n), TTR_E_INVALID, "ttr_qr_apply: kcols %lld > min(m, n)", (long long)kcols);
  return qr_apply_dispatch(dtype, m, n, batch, workspace, workspace_bytes, C, ldc, strideC, kcols, Out, ldo, strideO,
                           (hipStream_t)stream);
}

int ttr_qr(int dtype, int64_t m, int64_t n, int64_t batch, const void* A, int64_t lda, int64_t strideA, void* Q,
           int64_t ldq, int64_t strideQ, void* R, int64_t ldr, int64_t strideR, void* workspace,
           int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(Q != nullptr || batch == 0, TTR_E_INVALID, "ttr_qr: null pointer");
  int rc = ttr_qr_factor(dtype, m, n, batch, A, lda, strideA, R, ldr, strideR, workspace, workspace_bytes, stream);
  if (rc != TTR_OK || batch == 0) return rc;
  return ttr_qr_apply(dtype, m, n, batch, workspace, workspace_bytes, nullptr, 0, 0, m < n ? m : n, Q, ldq, strideQ,
                      stream);
}

int ttr_qr_t(int dtype, int64_t m, int64_t n, int64_t batch, const void* At, int64_t ldat, int64_t strideAt, void* Qt,
             int64_t ldqt, int64_t strideQt, void* R, int64_t ldr, int64_t strideR, void* workspace,
             int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_qr_t: bad dtype %d", dtype);
  TTR_REQUIRE(m >= 1 && n >= 1 && batch >= 0, TTR_E_INVALID, "ttr_qr_t: bad shape %lld x %lld", (long long)m, (long long)n);
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(At && Qt && R && workspace, TTR_E_INVALID, "ttr_qr_t: null pointer");
  TTR_REQUIRE(ldat >= m && ldqt >= m, TTR_E_INVALID, "ttr_qr_t: leading dimensions below m");
  // the factored matrix is A = At^T: element (row, col) at At[col * ldat + row]; Q^T goes out the same way
  int rc = qr_factor_dispatch(dtype, m, n, batch, At, 1, strideAt, R, ldr, strideR, workspace, workspace_bytes, (hipStream_t)stream, ldat);
  if (rc != TTR_OK) return rc;
  return qr_apply_dispatch(dtype, m, n, batch, workspace, workspace_bytes, nullptr, 0, 0, m < n ? m : n, Qt, 1, strideQt,
                           (hipStream_t)stream, ldqt);
}

int64_t ttr_qr_pushed_workspace_bytes(int dtype, int64_t I, int64_t n, int64_t batch) {
  return qr_pushed_workspace_bytes(dtype, I, n, batch);
}

int ttr_qr_factor_pushed(int dtype, int64_t k, int64_t Rin, int64_t I, int64_t n, int64_t batch, const void* Rm,
                         int64_t ldrm, int64_t strideRm, const void* core, int64_t stride_core, void* R, int64_t ldr,
                         int64_t strideR, void* workspace, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_qr_factor_pushed: bad dtype %d", dtype);
  TTR_REQUIRE(batch >= 0, TTR_E_INVALID, "ttr_qr_factor_pushed: negative batch");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(Rm && core && R && workspace, TTR_E_INVALID, "ttr_qr_factor_pushed: null pointer");
  return qr_factor_pushed_dispatch(dtype, k, Rin, I, n, batch, Rm, ldrm, strideRm, core, stride_core, R, ldr, strideR,
                                   workspace, workspace_bytes, (hipStream_t)stream);
}

int ttr_qr_factor_pushed_expo(int dtype, int64_t k, int64_t Rin, int64_t I, int64_t n, int64_t batch, const void* Rm,
                              int64_t ldrm, int64_t strideRm, const void* core, int64_t stride_core, void* R, int64_t ldr,
                              int64_t strideR, void* workspace, int64_t workspace_bytes, int32_t* expo_acc, void* stream) {
  TTR_REQUIRE(dtype == TTR_F32, TTR_E_UNSUPPORTED, "ttr_qr_factor_pushed_expo: fp32 only (dtype %d)", dtype);
  TTR_REQUIRE(batch >= 0, TTR_E_INVALID, "ttr_qr_factor_pushed_expo: negative batch");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(Rm && core && R && workspace && expo_acc, TTR_E_INVALID, "ttr_qr_factor_pushed_expo: null pointer");
  return qr_factor_pushed_dispatch(dtype, k, Rin, I, n, batch, Rm, ldrm, strideRm, core, stride_core, R, ldr, strideR,
                                   workspace, workspace_bytes, (hipStream_t)stream, expo_acc);
}

int ttr_qr_factor_pushed_sum(int dtype, int64_t k, int64_t I, int64_t batch, const void* Rm, int64_t ldrm,
                             int64_t strideRm, const void* core_a, int64_t ra, int64_t ca, int64_t stride_a,
                             const void* core_b, int64_t rb, int64_t cb, int64_t stride_b, void* R, int64_t ldr,
                             int64_t strideR, void* workspace, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_qr_factor_pushed_sum: bad dtype %d", dtype);
  TTR_REQUIRE(batch >= 0, TTR_E_INVALID, "ttr_qr_factor_pushed_sum: negative batch");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(Rm && core_a && core_b && R && workspace, TTR_E_INVALID, "ttr_qr_factor_pushed_sum: null pointer");
  return qr_factor_pushed_sum_dispatch(dtype, k, I, batch, Rm, ldrm, strideRm, core_a, ra, ca, stride_a, core_b, rb, cb,
                                       stride_b, R, ldr, strideR, workspace, workspace_bytes, (hipStream_t)stream);
}

int ttr_qr_apply_pushed(int dtype, int64_t k, int64_t I, int64_t n, int64_t batch, void* workspace,
                        int64_t workspace_bytes, const void* C, int64_t ldc, int64_t strideC, int64_t kcols, void* Out,
                        int64_t ldo, int64_t strideO, int skip_zero_rows, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_qr_apply_pushed: bad dtype %d", dtype);
  TTR_REQUIRE(batch >= 0 && kcols >= 1 && kcols <= n, TTR_E_INVALID, "ttr_qr_apply_pushed: bad arguments");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(Out && workspace, TTR_E_INVALID, "ttr_qr_apply_pushed: null pointer");
  return qr_apply_pushed_dispatch(dtype, k, I, n, batch, workspace, workspace_bytes, C, ldc, strideC, kcols, Out, ldo,
                                  strideO, nullptr, (hipStream_t)stream, skip_zero_rows ? 1 : 0);
}

int64_t ttr_qr_apply_pushed_gram_parts(int dtype, int64_t k, int64_t I, int64_t n, int64_t kcols) {
  if (!dtype_ok(dtype)) return 0;
  return qr_apply_pushed_gram_parts(dtype, k, I, n, kcols);
}

int ttr_qr_apply_pushed_gram(int dtype, int64_t k, int64_t I, int64_t n, int64_t batch, void* workspace,
                             int64_t workspace_bytes, const void* C, int64_t ldc, int64_t strideC, int64_t kcols,
                             void* Out, int64_t ldo, int64_t strideO, void* G, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_qr_apply_pushed_gram: bad dtype %d", dtype);
  TTR_REQUIRE(batch >= 0 && kcols >= 1 && kcols <= n, TTR_E_INVALID, "ttr_qr_apply_pushed_gram: bad arguments");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(Out && workspace && G, TTR_E_INVALID, "ttr_qr_apply_pushed_gram: null pointer");
  return qr_apply_pushed_dispatch(dtype, k, I, n, batch, workspace, workspace_bytes, C, ldc, strideC, kcols, Out, ldo,
                                  strideO, G, (hipStream_t)stream);
}

int64_t ttr_eigh_workspace_bytes(int dtype, int64_t n, int64_t batch) { return eigh_workspace_bytes(dtype, n, batch); }

static int eigh_trunc_checked(int dtype, int64_t n, int64_t batch, const void* G, int64_t ldg, int64_t strideG, int64_t gparts,
                              int64_t stride_gpart, void* V, int64_t ldv, int64_t strideV, void* sigma, int64_t stride_sigma,
                              int32_t* info, int eig_mode, int use_delta, double delta2, const double* delta2_dev, int64_t rmax,
                              int abs_floor, int32_t* sweeps, const int32_t* skip_items, const void* sigma_in,
                              int64_t stride_sigma_in, void* workspace, int64_t workspace_bytes, void* stream, int skip_lean) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_eigh_trunc: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 1 && batch >= 0 && rmax >= 1 && gparts >= 1, TTR_E_INVALID, "ttr_eigh_trunc: bad arguments");
  TTR_REQUIRE(abs_floor >= TTR_SOLVER_JACOBI_REL && abs_floor <= TTR_SOLVER_JACOBI_LIVE, TTR_E_INVALID,
              "ttr_eigh_trunc: bad solver %d", abs_floor);
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(G && V && sigma && info, TTR_E_INVALID, "ttr_eigh_trunc: null pointer");
  TTR_REQUIRE(eig_mode >= TTR_EIG_RAW && eig_mode <= TTR_EIG_MATCH_DIAG, TTR_E_INVALID, "ttr_eigh_trunc: bad eig_mode %d",
              eig_mode);
  return eigh_dispatch(dtype, n, batch, G, ldg, strideG, gparts, stride_gpart, V, ldv, strideV, sigma, stride_sigma, info,
                       eig_mode, use_delta, delta2, rmax, abs_floor, sweeps, workspace, workspace_bytes,
                       (hipStream_t)stream, delta2_dev, skip_items, sigma_in, stride_sigma_in, skip_lean);
}

int ttr_eigh_trunc(int dtype, int64_t n, int64_t batch, const void* G, int64_t ldg, int64_t strideG, int64_t gparts,
                   int64_t stride_gpart, void* V, int64_t ldv, int64_t strideV, void* sigma, int64_t stride_sigma,
                   int32_t* info, int eig_mode, int use_delta, double delta2, const double* delta2_dev, int64_t rmax,
                   int abs_floor, int32_t* sweeps, const int32_t* skip_items, const void* sigma_in, int64_t stride_sigma_in,
                   void* workspace, int64_t workspace_bytes, void* stream) {
  return eigh_trunc_checked(dtype, n, batch, G, ldg, strideG, gparts, stride_gpart, V, ldv, strideV, sigma, stride_sigma, info,
                            eig_mode, use_delta, delta2, delta2_dev, rmax, abs_floor, sweeps, skip_items, sigma_in,
                            stride_sigma_in, workspace, workspace_bytes, stream, 0);
}

int ttr_eigh_trunc_pass(int dtype, int64_t n, int64_t batch, const void* G, int64_t ldg, int64_t strideG, int64_t gparts,
                        int64_t stride_gpart, void* V, int64_t ldv, int64_t strideV, void* sigma, int64_t stride_sigma,
                        int32_t* info, int eig_mode, int use_delta, double delta2, const double* delta2_dev, int64_t rmax,
                        int abs_floor, int32_t* sweeps, const int32_t* skip_items, const void* sigma_in,
                        int64_t stride_sigma_in, void* workspace, int64_t workspace_bytes, void* stream) {
  return eigh_trunc_checked(dtype, n, batch, G, ldg, strideG, gparts, stride_gpart, V, ldv, strideV, sigma, stride_sigma, info,
                            eig_mode, use_delta, delta2, delta2_dev, rmax, abs_floor, sweeps, skip_items, sigma_in,
                            stride_sigma_in, workspace, workspace_bytes, stream, 1);
}

int ttr_eigh_top_ok(int64_t n, int64_t r) { return n >= 40 && n <= 64 && r >= 1 && r <= 32 && r < n; }

int ttr_eigh_top(int dtype, int64_t n, int64_t batch, const void* G, int64_t ldg, int64_t strideG, int64_t gparts,
                 int64_t stride_gpart, void* V, int64_t ldv, int64_t strideV, void* sigma, int64_t stride_sigma, int32_t* info,
                 int64_t r, double thr, int32_t* flat, int need_all, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_eigh_top: bad dtype %d", dtype);
  TTR_REQUIRE(batch >= 0 && gparts >= 1 && thr > 0.0 && thr <= 1.0, TTR_E_INVALID, "ttr_eigh_top: bad arguments");
  TTR_REQUIRE(ttr_eigh_top_ok(n, r), TTR_E_UNSUPPORTED, "ttr_eigh_top: n = %lld, r = %lld outside 40 <= n <= 64, r <= 32, r < n",
              (long long)n, (long long)r);
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(G && V && sigma && info, TTR_E_INVALID, "ttr_eigh_top: null pointer");
  return eigh_top_dispatch(dtype, n, batch, G, ldg, strideG, gparts, stride_gpart, V, ldv, strideV, sigma, stride_sigma, info, r, thr,
                           flat, (hipStream_t)stream, need_all);
}

int64_t ttr_bj_scratch_bytes(int dtype, int64_t b, int64_t npairs, int64_t items) {
  const int64_t elem = dtype == TTR_F64 ? 8 : 4;
  return items * npairs * (2 * b + 1) * elem;
}

static int bj_ok(const char* who, int dtype, int64_t b, int64_t npairs, int64_t items) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "%s: bad dtype %d", who, dtype);
  TTR_REQUIRE(b >= 1 && b <= 32 && npairs >= 1 && npairs <= 65535 && items >= 0, TTR_E_UNSUPPORTED,
              "%s: block width %lld outside [1, 32] or %lld pairs outside [1, 65535]", who, (long long)b, (long long)npairs);
  return TTR_OK;
}

int ttr_bj_solve(int dtype, int64_t b, int64_t npairs, int64_t items, const void* G, int64_t ldg, int64_t strideG,
                 const int32_t* pair_tab, void* W, void* scratch, int32_t* ctrl, void* stream) {
  const int rc = bj_ok("ttr_bj_solve", dtype, b, npairs, items);
  if (rc != TTR_OK) return rc;
  if (items == 0) return TTR_OK;
  TTR_REQUIRE(G && pair_tab && W && scratch && ctrl, TTR_E_INVALID, "ttr_bj_solve: null pointer");
  TTR_REQUIRE(items * npairs < (int64_t(1) << 31), TTR_E_UNSUPPORTED, "ttr_bj_solve: %lld pair problems exceed the grid",
              (long long)(items * npairs));
  return eigh_pairs_dispatch(dtype, b, npairs, items, G, ldg, strideG, pair_tab, W, scratch, ctrl, ctrl + 1, (hipStream_t)stream);
}

int ttr_bj_apply(int dtype, int64_t b, int64_t npairs, int64_t items, void* G, int64_t ldg, int64_t strideG, void* V,
                 int64_t ldv, int64_t strideV, const int32_t* pair_tab, const void* W, const int32_t* ctrl, double* offsq,
                 void* stream) {
  const int rc = bj_ok("ttr_bj_apply", dtype, b, npairs, items);
  if (rc != TTR_OK) return rc;
  if (items == 0) return TTR_OK;
  TTR_REQUIRE(G && V && pair_tab && W && ctrl, TTR_E_INVALID, "ttr_bj_apply: null pointer");
  return bj_apply_dispatch(dtype, b, npairs, items, G, ldg, strideG, V, ldv, strideV, pair_tab, W, ctrl, offsq, (hipStream_t)stream);
}

int ttr_bj_control(int dtype, int64_t items, int32_t* ctrl, double* state, const void* gnorm, int relative, double tol,
                   void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_bj_control: bad dtype %d", dtype);
  TTR_REQUIRE(ctrl && state && (relative || gnorm), TTR_E_INVALID, "ttr_bj_control: null pointer");
  return bj_control_dispatch(dtype, items, ctrl, state, gnorm, relative, tol, (hipStream_t)stream);
}

int64_t ttr_sweep_gram_parts(int64_t n, int64_t batch) {
  if (n <= 0 || batch <= 0) return 1;
  return sweep_gram_parts(n, batch);
}

int ttr_rowgram(int dtype, int64_t R, int64_t n, int64_t batch, const void* M, int64_t ldm, int64_t strideM, void* G,
                int64_t nparts, const int32_t* rows32, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_rowgram: bad dtype %d", dtype);
  TTR_REQUIRE(R >= 1 && n >= 1 && batch >= 0, TTR_E_INVALID, "ttr_rowgram: bad shape");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(M && G, TTR_E_INVALID, "ttr_rowgram: null pointer");
  return sweep_gram_dispatch(dtype, R, n, batch, M, ldm, strideM, nullptr, 0, 0, G, nparts, (hipStream_t)stream, nullptr, rows32);
}

int64_t ttr_qr_pushed_flag_offset(int dtype, int64_t I, int64_t n, int64_t batch) {
  if (!dtype_ok(dtype) || I < 1 || n < 1 || batch < 1) return -1;
  return qr_pushed_flag_offset(dtype, I, n, batch);
}

int ttr_rotgram(int dtype, int64_t R, int64_t n, int64_t batch, const void* M, int64_t ldm, int64_t strideM,
                const void* V1, int64_t ldv1, int64_t strideV1, void* G, int64_t nparts, const int32_t* skip,
                const int32_t* rows32, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_rotgram: bad dtype %d", dtype);
  TTR_REQUIRE(R >= 1 && n >= 1 && batch >= 0, TTR_E_INVALID, "ttr_rotgram: bad shape");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(M && G && V1, TTR_E_INVALID, "ttr_rotgram: null pointer");
  return sweep_gram_dispatch(dtype, R, n, batch, M, ldm, strideM, V1, ldv1, strideV1, G, nparts, (hipStream_t)stream, skip, rows32);
}

int ttr_eigsel_max_n(void) { return eigsel_max_n(); }

int64_t ttr_eigsel_scratch_bytes(int dtype, int64_t n, int64_t batch) {
  if (!dtype_ok(dtype) || n < 1 || batch < 0) return -1;
  return eigsel_scratch_bytes(dtype, n, batch);
}

int64_t ttr_tridiag_workspace_bytes(int dtype, int64_t n, int64_t batch) {
  if (!dtype_ok(dtype) || n < 1 || batch < 0) return -1;
  return tridiag_workspace_bytes(dtype, n, batch);
}

int ttr_tridiag(int dtype, int64_t n, int64_t batch, void* A, int64_t lda, int64_t strideA, void* d, void* e, void* tau,
                void* workspace, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_tridiag: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 2 && n <= eigsel_max_n(), TTR_E_UNSUPPORTED, "ttr_tridiag: n = %lld outside [2, %d]", (long long)n, eigsel_max_n());
  TTR_REQUIRE(batch >= 0 && lda >= n, TTR_E_INVALID, "ttr_tridiag: bad shape");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(A && d && e && tau, TTR_E_INVALID, "ttr_tridiag: null pointer");
  TTR_REQUIRE(!workspace || workspace_bytes >= tridiag_workspace_bytes(dtype, n, batch), TTR_E_WORKSPACE,
              "ttr_tridiag: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)tridiag_workspace_bytes(dtype, n, batch));
  return tridiag_dispatch(dtype, n, batch, A, lda, strideA, d, e, tau, workspace, (hipStream_t)stream);
}

int ttr_tri_eigsel(int dtype, int64_t n, int64_t batch, int64_t k, const void* d, const void* e, void* lam, void* Z, void* scratch,
                   int64_t scratch_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_tri_eigsel: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 2 && n <= eigsel_max_n() && k >= 1 && k <= 64 && k <= n, TTR_E_UNSUPPORTED,
              "ttr_tri_eigsel: n = %lld, k = %lld outside n in [2, %d], k in [1, min(64, n)]", (long long)n, (long long)k, eigsel_max_n());
  TTR_REQUIRE(batch >= 0, TTR_E_INVALID, "ttr_tri_eigsel: bad batch");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(d && e && lam && Z && scratch, TTR_E_INVALID, "ttr_tri_eigsel: null pointer");
  TTR_REQUIRE(scratch_bytes >= eigsel_scratch_bytes(dtype, n, batch), TTR_E_WORKSPACE, "ttr_tri_eigsel: scratch %lld < %lld bytes",
              (long long)scratch_bytes, (long long)eigsel_scratch_bytes(dtype, n, batch));
  return eigsel_dispatch(dtype, n, batch, k, d, e, lam, Z, scratch, (hipStream_t)stream);
}

int ttr_tridiag_back(int dtype, int64_t n, int64_t batch, int64_t k, const void* A, int64_t lda, int64_t strideA, const void* tau,
                     void* Z, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_tridiag_back: bad dtype %d", dtype);
  TTR_REQUIRE(n >= 2 && n <= eigsel_max_n() && k >= 1 && k <= 64, TTR_E_UNSUPPORTED, "ttr_tridiag_back: n = %lld, k = %lld unsupported",
              (long long)n, (long long)k);
  TTR_REQUIRE(batch >= 0 && lda >= n, TTR_E_INVALID, "ttr_tridiag_back: bad shape");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(A && tau && Z, TTR_E_INVALID, "ttr_tridiag_back: null pointer");
  return tridiag_back_dispatch(dtype, n, batch, k, A, lda, strideA, tau, Z, (hipStream_t)stream);
}

int ttr_project_flat(int dtype, int64_t R, int64_t n, int64_t ro, int64_t batch, const void* M, int64_t ldm, int64_t strideM,
                     const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2, int64_t strideV2,
                     const void* sigma, int64_t stride_sigma, int scale_right, void* right, int64_t ldr, int64_t strideR,
                     void* left, int64_t ldl, int64_t strideL, const int32_t* rows32, const int32_t* flat, const void* sigma1,
                     int64_t stride_sigma1, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_project: bad dtype %d", dtype);
  // (ro outside [1, R] is a matter of the kernels' envelope: TTR_E_UNSUPPORTED from the dispatcher, like ro > R)
  TTR_REQUIRE(R >= 1 && n >= 1 && batch >= 0, TTR_E_INVALID, "ttr_project: bad shape");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(M && V2 && right, TTR_E_INVALID, "ttr_project: null pointer");
  TTR_REQUIRE(!scale_right || sigma, TTR_E_INVALID, "ttr_project: scale_right needs sigma");
  TTR_REQUIRE(!flat || !V1 || sigma1, TTR_E_INVALID, "ttr_project_flat: flat needs sigma1");
  return sweep_project_dispatch(dtype, R, n, ro, batch, M, ldm, strideM, V1, ldv1, strideV1, V2, ldv2, strideV2, sigma,
                                stride_sigma, scale_right, right, ldr, strideR, left, ldl, strideL, (hipStream_t)stream, rows32,
                                flat, sigma1, stride_sigma1);
}

int ttr_project(int dtype, int64_t R, int64_t n, int64_t ro, int64_t batch, const void* M, int64_t ldm, int64_t strideM,
                const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2, int64_t strideV2,
                const void* sigma, int64_t stride_sigma, int scale_right, void* right, int64_t ldr, int64_t strideR,
                void* left, int64_t ldl, int64_t strideL, const int32_t* rows32, void* stream) {
  return ttr_project_flat(dtype, R, n, ro, batch, M, ldm, strideM, V1, ldv1, strideV1, V2, ldv2, strideV2, sigma, stride_sigma,
                          scale_right, right, ldr, strideR, left, ldl, strideL, rows32, nullptr, nullptr, 0, stream);
}

int64_t ttr_colgram_workspace_bytes(int dtype, int64_t rows, int64_t n, int64_t batch) {
  if (rows <= 0 || n <= 0 || batch <= 0) return 0;
  return colgram_workspace_bytes(dtype, rows, n, batch);
}

int ttr_colgram(int dtype, int64_t rows, int64_t n, int64_t batch, const void* M, int64_t ldm, int64_t strideM,
                const void* V1, int64_t ldv1, int64_t strideV1, void* G, void* workspace, int64_t workspace_bytes,
                const int32_t* skip, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_colgram: bad dtype %d", dtype);
  TTR_REQUIRE(rows >= 1 && n >= 1 && batch >= 0, TTR_E_INVALID, "ttr_colgram: bad shape");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(M && G, TTR_E_INVALID, "ttr_colgram: null pointer");
  return colgram_dispatch(dtype, rows, n, batch, M, ldm, strideM, V1, ldv1, strideV1, G, workspace, workspace_bytes,
                          (hipStream_t)stream, skip);
}

int ttr_colproject(int dtype, int64_t rows, int64_t n, int64_t ro, int64_t batch, const void* M, int64_t ldm,
                   int64_t strideM, const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2,
                   int64_t strideV2, const void* sigma, int64_t stride_sigma, int left_ortho, void* left, int64_t ldl,
                   int64_t strideL, void* right, int64_t ldr, int64_t strideR, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_colproject: bad dtype %d", dtype);
  TTR_REQUIRE(rows >= 1 && n >= 1 && batch >= 0, TTR_E_INVALID, "ttr_colproject: bad shape");   // (ro: as ttr_project's)
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(M && V2 && left, TTR_E_INVALID, "ttr_colproject: null pointer");
  TTR_REQUIRE(!left_ortho || sigma, TTR_E_INVALID, "ttr_colproject: left_ortho needs sigma");
  return colproject_dispatch(dtype, rows, n, ro, batch, M, ldm, strideM, V1, ldv1, strideV1, V2, ldv2, strideV2, sigma,
                             stride_sigma, left_ortho, left, ldl, strideL, right, ldr, strideR, (hipStream_t)stream);
}

int ttr_krp_contract(int dtype, int64_t P, int64_t J, int64_t Q, int64_t R, const void* T, const void* B, int64_t ldb,
                     void* out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_krp_contract: bad dtype %d", dtype);
  TTR_REQUIRE(P >= 0 && J >= 1 && Q >= 0 && R >= 1 && ldb >= R, TTR_E_INVALID, "ttr_krp_contract: bad sizes");
  if (P == 0 || Q == 0) return TTR_OK;
  TTR_REQUIRE(T && B && out, TTR_E_INVALID, "ttr_krp_contract: null pointer");
  return krp_contract_dispatch(dtype, P, J, Q, R, T, B, ldb, out, (hipStream_t)stream);
}

int ttr_hadamard(int dtype, int64_t count, const void* a, const void* b, void* out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_hadamard: bad dtype %d", dtype);
  TTR_REQUIRE(count >= 0, TTR_E_INVALID, "ttr_hadamard: negative count");
  if (count == 0) return TTR_OK;
  TTR_REQUIRE(a && b && out, TTR_E_INVALID, "ttr_hadamard: null pointer");
  return hadamard_dispatch(dtype, count, a, b, out, (hipStream_t)stream);
}

int ttr_core_kron(int dtype, int64_t batch, int64_t R1, int64_t S1, int64_t I, int64_t R2, int64_t S2, const void* a,
                  const void* c, void* out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_core_kron: bad dtype %d", dtype);
  TTR_REQUIRE(batch >= 0 && R1 >= 1 && S1 >= 1 && I >= 1 && R2 >= 1 && S2 >= 1, TTR_E_INVALID, "ttr_core_kron: bad sizes");
  if (batch == 0) return TTR_OK;
  TTR_REQUIRE(a && c && out, TTR_E_INVALID, "ttr_core_kron: null pointer");
  return core_kron_dispatch(dtype, batch, R1, S1, I, R2, S2, a, c, out, (hipStream_t)stream);
}

int ttr_debug_set_qr_stamps(void* device_buffer) {
  g_qr_dbg = (long long*)device_buffer;
  return TTR_OK;
}

int ttr_debug_set_knob(int knob, int value) {
  switch (knob) {
    case TTR_KNOB_QR_STAMP_BX:
      g_qr_dbg_bx = value;
      return TTR_OK;
    case TTR_KNOB_QR_STAMP_BY:
      g_qr_dbg_by = value;
      return TTR_OK;
    case TTR_KNOB_EIGH_SMALL:
      TTR_REQUIRE(value >= 0 && value <= 3, TTR_E_INVALID, "ttr_debug_set_knob: small-eigensolver switch %d outside [0, 3]", value);
      g_eigh_small = value;
      return TTR_OK;
    case TTR_KNOB_ORTH_SPLIT:
      TTR_REQUIRE(value >= 0 && value <= 65535, TTR_E_INVALID, "ttr_debug_set_knob: orth split threshold %d outside [0, 65535]", value);
      g_orth_split = value;
      return TTR_OK;
    case TTR_KNOB_SWEEP_STAGGER:
      TTR_REQUIRE(value >= 0 && value <= 2, TTR_E_INVALID, "ttr_debug_set_knob: stagger mode %d outside [0, 2]", value);
      g_sweep_stagger = value;
      return TTR_OK;
    case TTR_KNOB_FLAT_PASS:
      TTR_REQUIRE(value >= 0 && value <= 1, TTR_E_INVALID, "ttr_debug_set_knob: flat pass-through switch %d outside [0, 1]", value);
      g_flat_pass = value;
      return TTR_OK;
    case TTR_KNOB_SWEEP_LEAN:
      TTR_REQUIRE(value >= 0 && value <= 1, TTR_E_INVALID, "ttr_debug_set_knob: lean sweep switch %d outside [0, 1]", value);
      g_sweep_lean = value;
      return TTR_OK;
    case TTR_KNOB_EIGH_BIG_OCC:
      TTR_REQUIRE(value == 0 || value == 2 || value == 3, TTR_E_INVALID, "ttr_debug_set_knob: eigensolver occupancy %d not in {0, 2, 3}", value);
      g_eigh_big_occ = value;
      return TTR_OK;
    case TTR_KNOB_QR_PACK_PRE:
      TTR_REQUIRE(value >= 0 && value <= 3, TTR_E_INVALID, "ttr_debug_set_knob: pack-flag switch %d outside [0, 3]", value);
      g_qr_pack_pre = value & 1;
      g_qr_l1_idle = (value & 2) ? 0 : 1;
      return TTR_OK;
    case TTR_KNOB_QR_PAIR4:
      TTR_REQUIRE(value >= 0 && value <= 3, TTR_E_INVALID, "ttr_debug_set_knob: four-wave pair switch %d outside [0, 3]", value);
      g_qr_pair4 = value;
      return TTR_OK;
    case TTR_KNOB_QR_STAGGER:
      TTR_REQUIRE(value >= 0 && value <= 1024, TTR_E_INVALID, "ttr_debug_set_knob: stagger of %d kilo-cycles outside [0, 1024]", value);
      g_qr_stagger = value;
      return TTR_OK;
    case TTR_KNOB_QR_INTERLEAVE:
      TTR_REQUIRE(value >= 0 && value <= 1, TTR_E_INVALID, "ttr_debug_set_knob: interleave switch %d outside [0, 1]", value);
      g_qr_interleave = value;
      return TTR_OK;
    case TTR_KNOB_ORTH_V2:
      TTR_REQUIRE(value >= 0 && value <= 2, TTR_E_INVALID, "ttr_debug_set_knob: orth_fixup variant %d outside [0, 2]", value);
      g_orth_v2 = value;
      return TTR_OK;
    case TTR_KNOB_JACOBI_LIVE_WAVE:
      TTR_REQUIRE(value >= 0 && value <= 1, TTR_E_INVALID, "ttr_debug_set_knob: pass-2 Jacobi switch %d outside [0, 1]", value);
      g_jacobi_live_wave = value;
      return TTR_OK;
    case TTR_KNOB_ORTH_ROUNDS:
      TTR_REQUIRE(value >= 1 && value <= 4, TTR_E_INVALID, "ttr_debug_set_knob: %d rounds outside [1, 4]", value);
      g_orth_rounds = value;
      return TTR_OK;
    case TTR_KNOB_RANK_NOISE_FLOOR:
      TTR_REQUIRE(value >= 0 && value <= 1024, TTR_E_INVALID, "ttr_debug_set_knob: rank-rule noise floor %d outside [0, 1024]", value);
      g_rank_noise_c = value;
      return TTR_OK;
    case TTR_KNOB_QR_PACK:
      TTR_REQUIRE(value >= 0 && value <= 3, TTR_E_INVALID, "ttr_debug_set_knob: packing switch %d outside [0, 3]", value);
      g_qr_pack = value;
      return TTR_OK;
    case TTR_KNOB_QR_RANK_SKIP:
      TTR_REQUIRE(value >= 0 && value <= 4096, TTR_E_INVALID, "ttr_debug_set_knob: rank-skip factor %d outside [0, 4096]", value);
      g_rank_skip_c = value;
      return TTR_OK;
    case TTR_KNOB_QR_F64_NW4:
      TTR_REQUIRE(value >= 0 && value <= 7, TTR_E_INVALID, "ttr_debug_set_knob: 4-wave block switch %d outside [0, 7]", value);
      g_qr_f64_nw4 = value;
      return TTR_OK;
    case TTR_KNOB_GEMM_BIG:
      TTR_REQUIRE(value >= 0 && value <= 1, TTR_E_INVALID, "ttr_debug_set_knob: big-tile GEMM switch %d outside [0, 1]", value);
      g_gemm_big = value;
      return TTR_OK;
    case TTR_KNOB_BJ_INNER_SWEEPS:
      TTR_REQUIRE(value >= 0 && value <= 64, TTR_E_INVALID, "ttr_debug_set_knob: %d inner sweeps outside [0, 64]", value);
      g_bj_inner_sweeps = value;
      return TTR_OK;
    case TTR_KNOB_QR_PANEL:
      TTR_REQUIRE(value >= 0 && value <= 1, TTR_E_INVALID, "ttr_debug_set_knob: QR panel variant %d outside [0, 1]", value);
      g_qr_variant = value;
      return TTR_OK;
    default:
      TTR_REQUIRE(false, TTR_E_INVALID, "ttr_debug_set_knob: unknown knob %d", knob);
  }
}

int ttr_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
  g_prof_level = on;
  if (on >= 2) {   // census mode: per-kind device counters (the only allocation this library ever makes; profiling runs only)
    if (!g_work_dev) TTR_HIP_CHECK(hipMalloc((void**)&g_work_dev, 2 * TTR_PROF_NKINDS * sizeof(double)));
    TTR_HIP_CHECK(hipMemset(g_work_dev, 0, 2 * TTR_PROF_NKINDS * sizeof(double)));
  }
  return TTR_OK;
}

int ttr_prof_collect(double* ms, int64_t* launches) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int k = 0; k < TTR_PROF_NKINDS; ++k) {
    if (ms) ms[k] = 0.0;
    if (launches) launches[k] = 0;
  }
  for (auto& r : g_prof_recs) {
    if (hipEventSynchronize(r.stop) == hipSuccess) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, r.start, r.stop) == hipSuccess && r.kind >= 0 && r.kind < TTR_PROF_NKINDS) {
        if (ms) ms[r.kind] += (double)t;
        if (launches) launches[r.kind] += 1;
      }
    }
    g_prof_pool.push_back({r.start, r.stop});
  }
  g_prof_recs.clear();
  return TTR_OK;
}

int ttr_prof_collect_work(double* flops, double* bytes) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double host[2 * TTR_PROF_NKINDS] = {0};
  if (g_work_dev) {
    TTR_HIP_CHECK(hipDeviceSynchronize());
    TTR_HIP_CHECK(hipMemcpy(host, g_work_dev, sizeof(host), hipMemcpyDeviceToHost));
    TTR_HIP_CHECK(hipMemset(g_work_dev, 0, sizeof(host)));
  }
  for (int k = 0; k < TTR_PROF_NKINDS; ++k) {
    if (flops) flops[k] = host[k];
    if (bytes) bytes[k] = host[TTR_PROF_NKINDS + k];
  }
  return TTR_OK;
}

}  // extern "C"
