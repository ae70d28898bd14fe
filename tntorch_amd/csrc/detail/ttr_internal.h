// What the translation units of libttround_hip.so share on the host and ttr_common.h does not hold: the prototypes of the
// dispatchers the extern "C" wrappers call, the knob globals ttr_debug_set_knob writes, and the host helpers of the entries
// (dtype checks and dispatch, stride and alignment tests, the argument checks of a core [R, I, C], the grid cap and the choice
// of pack widths of the tile kernels).
//
// HOST-ONLY: no __global__ / __device__ code and no template a kernel instantiates.  Including this file therefore cannot
// alter any kernel, which is why it may live outside the set of files bench.py hashes (csrc/*.h and the kernel sources:
// `source_sha` / `KIND_SOURCES`, which tie the counters of profiles/pmc_latest.json to the build they were taken from).
// What device code shares (Pack, block_sum, the wave reductions) lives in ttr_common.h.
//
// Included by EVERY .hip file of the library: a unit that defines a dispatcher or a knob declared here has its definition
// checked against the declaration by the compiler (default arguments stand here, on the declaration, only), and a unit with
// extern "C" entries takes its checks and its dtype dispatch from the helpers at the end instead of carrying copies.
#pragma once
#include <type_traits>

#include "../ttr_common.h"

namespace ttr {

// ------------------------------------------------------------------ dispatchers (ttr_gemm / ttr_cp / ttr_qr / ttr_eigh / ttr_bjacobi /
// ttr_eigsel / ttr_sweep .hip)
int gemm_dispatch(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                  int64_t strideA, const void* B, int64_t ldb, int64_t strideB, void* C, int64_t ldc, int64_t strideC,
                  const void* rs, int64_t stride_rs, int rs_mode, const void* cs, int64_t stride_cs, int cs_mode,
                  int64_t batch, void* ws, int64_t ws_bytes, hipStream_t stream, int axpby = 0, double alpha = 1.0,
                  double beta = 0.0);
int64_t gemm_workspace_bytes(int dtype, int64_t M, int64_t N, int64_t K, int64_t batch);
int krp_contract_dispatch(int dtype, int64_t P, int64_t J, int64_t Q, int64_t R, const void* Tn, const void* B,
                          int64_t ldb, void* out, hipStream_t stream);
int hadamard_dispatch(int dtype, int64_t count, const void* a, const void* b, void* out, hipStream_t stream);
int core_kron_dispatch(int dtype, int64_t B, int64_t R1, int64_t S1, int64_t I, int64_t R2, int64_t S2, const void* a,
                       const void* c, void* out, hipStream_t stream);
int qr_factor_dispatch(int dtype, int64_t m, int64_t n, int64_t batch, const void* A, int64_t lda, int64_t strideA,
                       void* R, int64_t ldr, int64_t strideR, void* ws, int64_t ws_bytes, hipStream_t stream, int64_t a_cs = 1,
                       int32_t* expo_acc = nullptr);
int qr_apply_dispatch(int dtype, int64_t m, int64_t n, int64_t batch, void* ws, int64_t ws_bytes, const void* C,
                      int64_t ldc, int64_t strideC, int64_t kc, void* Out, int64_t ldo, int64_t strideO,
                      hipStream_t stream, int64_t o_cs = 1);
int64_t qr_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t batch);
int64_t qr_pushed_workspace_bytes(int dtype, int64_t I, int64_t n, int64_t batch);
int qr_factor_pushed_dispatch(int dtype, int64_t k, int64_t Rin, int64_t I, int64_t n, int64_t batch, const void* Rm,
                              int64_t ldrm, int64_t strideRm, const void* Cn, int64_t strideCn, void* R, int64_t ldr,
                              int64_t strideR, void* ws, int64_t ws_bytes, hipStream_t stream, int32_t* expo_acc = nullptr);
int qr_factor_pushed_sum_dispatch(int dtype, int64_t k, int64_t I, int64_t batch, const void* Rm, int64_t ldrm,
                                  int64_t strideRm, const void* Ca, int64_t ra, int64_t ca, int64_t strideCa,
                                  const void* Cb, int64_t rb, int64_t cb, int64_t strideCb, void* R, int64_t ldr,
                                  int64_t strideR, void* ws, int64_t ws_bytes, hipStream_t stream);
int qr_apply_pushed_dispatch(int dtype, int64_t k, int64_t I, int64_t n, int64_t batch, void* ws, int64_t ws_bytes,
                             const void* C, int64_t ldc, int64_t strideC, int64_t kc, void* Out, int64_t ldo,
                             int64_t strideO, void* G, hipStream_t stream, int skip_zero_rows = 0);
int64_t qr_apply_pushed_gram_parts(int dtype, int64_t k, int64_t I, int64_t n, int64_t kc);
int qr_max_cols(int dtype);
int eigh_dispatch(int dtype, int64_t n, int64_t batch, const void* G, int64_t ldg, int64_t strideG, int64_t gparts,
                  int64_t stride_gpart, void* V, int64_t ldv, int64_t strideV, void* sigma, int64_t stride_sigma, int32_t* info, int eig_mode,
                  int use_delta, double delta2, int64_t rmax, int abs_floor, int32_t* sweeps, void* ws,
                  int64_t ws_bytes, hipStream_t stream, const double* delta2_dev = nullptr, const int32_t* skip_items = nullptr,
                  const void* sigma_in = nullptr, int64_t stride_sigma_in = 0, int skip_lean = 0);
int eigh_top_dispatch(int dtype, int64_t n, int64_t batch, const void* G, int64_t ldg, int64_t strideG, int64_t gparts,
                      int64_t stride_gpart, void* V, int64_t ldv, int64_t strideV, void* sigma, int64_t stride_sigma, int32_t* info,
                      int64_t r, double thr, int32_t* flat, hipStream_t stream, int need_all);
int eigh_pairs_dispatch(int dtype, int64_t b, int64_t npairs, int64_t items, const void* G, int64_t ldg, int64_t strideG,
                        const int32_t* pair_tab, void* W, void* scratch, const int32_t* skip_flag, int32_t* rot_count,
                        hipStream_t stream);
int bj_apply_dispatch(int dtype, int64_t b, int64_t npairs, int64_t items, void* G, int64_t ldg, int64_t strideG, void* V,
                      int64_t ldv, int64_t strideV, const int32_t* pair_tab, const void* W, const int32_t* ctrl, double* offsq,
                      hipStream_t stream);
int bj_control_dispatch(int dtype, int64_t items, int32_t* ctrl, double* state, const void* gnorm, int relative, double tol,
                        hipStream_t stream);
int64_t eigsel_scratch_bytes(int dtype, int64_t n, int64_t batch);
int eigsel_max_n();
int64_t tridiag_workspace_bytes(int dtype, int64_t n, int64_t batch);
int tridiag_dispatch(int dtype, int64_t n, int64_t batch, void* A, int64_t lda, int64_t strideA, void* d, void* e, void* tau,
                     void* ws, hipStream_t stream);
int eigsel_dispatch(int dtype, int64_t n, int64_t batch, int64_t k, const void* d, const void* e, void* lam, void* Z, void* scratch,
                    hipStream_t stream);
int tridiag_back_dispatch(int dtype, int64_t n, int64_t batch, int64_t k, const void* A, int64_t lda, int64_t strideA, const void* tau,
                          void* Z, hipStream_t stream);
int64_t eigh_workspace_bytes(int dtype, int64_t n, int64_t batch);
int eigh_max_n(int dtype);
int eigh_max_n_lds(int dtype);

int sweep_gram_parts(int64_t n, int64_t batch);
int sweep_gram_dispatch(int dtype, int64_t R, int64_t n, int64_t batch, const void* Mx, int64_t ldm, int64_t strideM,
                        const void* V1, int64_t ldv1, int64_t strideV1, void* G, int64_t nsplit, hipStream_t stream,
                        const int32_t* skip = nullptr, const int32_t* rows32 = nullptr);
int sweep_project_dispatch(int dtype, int64_t R, int64_t n, int64_t ro, int64_t batch, const void* Mx, int64_t ldm,
                           int64_t strideM, const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2,
                           int64_t strideV2, const void* sigma, int64_t stride_sigma, int scale_right, void* right,
                           int64_t ldr, int64_t strideR, void* left, int64_t ldl, int64_t strideL, hipStream_t stream,
                           const int32_t* rows32 = nullptr, const int32_t* flat = nullptr, const void* sigma1 = nullptr,
                           int64_t stride_sigma1 = 0);
int64_t qr_pushed_flag_offset(int dtype, int64_t I, int64_t n, int64_t batch);

int64_t colgram_workspace_bytes(int dtype, int64_t rows, int64_t n, int64_t batch);
int colgram_dispatch(int dtype, int64_t rows, int64_t n, int64_t batch, const void* Mx, int64_t ldm, int64_t strideM,
                     const void* V1, int64_t ldv1, int64_t strideV1, void* G, void* ws, int64_t ws_bytes, hipStream_t stream,
                     const int32_t* skip = nullptr);
int colproject_dispatch(int dtype, int64_t rows, int64_t n, int64_t ro, int64_t batch, const void* Mx, int64_t ldm,
                        int64_t strideM, const void* V1, int64_t ldv1, int64_t strideV1, const void* V2, int64_t ldv2,
                        int64_t strideV2, const void* sigma, int64_t stride_sigma, int left_ortho, void* left, int64_t ldl,
                        int64_t strideL, void* right, int64_t ldr, int64_t strideR, hipStream_t stream);

// ------------------------------------------------------------------ knobs (ttr_debug_set_knob, ttr_debug_set_qr_stamps); defined where they are read
extern long long* g_qr_dbg;
extern int g_qr_variant;
extern int g_bj_inner_sweeps;
extern int g_gemm_big;
extern int g_qr_dbg_bx, g_qr_dbg_by;
extern int g_qr_f64_nw4;
extern int g_rank_skip_c;
extern int g_qr_pack;
extern int g_qr_interleave;
extern int g_qr_stagger;
extern int g_qr_pack_pre;
extern int g_qr_l1_idle;
extern int g_qr_pair4;
extern int g_eigh_big_occ;
extern int g_sweep_stagger;
extern int g_sweep_lean;
extern int g_flat_pass;
extern int g_rank_noise_c;
extern int g_jacobi_live_wave;
extern int g_eigh_small;
extern int g_orth_rounds, g_orth_v2, g_orth_split;   // ttr_orth.hip

// the census counters of ttr_prof_enable(2) ([2 * TTR_PROF_NKINDS]: flops per kind, then bytes per kind) for kernels that count
// their own work; nullptr unless work_census_on()
double* work_census_dev();

// ------------------------------------------------------------------ host helpers of the extern "C" entries
inline bool dtype_ok(int dtype) { return dtype == TTR_F32 || dtype == TTR_F64; }
inline int64_t elem_size(int dtype) { return dtype == TTR_F32 ? 4 : 8; }  // bytes; of a dtype that passed dtype_ok

// f(float{}) or f(double{}), and what it returns: for an entry whose two dtypes run the float or the double instance of ONE
// template with the same arguments (`using T = decltype(t)` inside the generic lambda)
template <typename F>
auto by_dtype(int dtype, F&& f) -> decltype(f(float{})) {
  if (dtype == TTR_F32) return f(float{});
  return f(double{});
}

// element strides of a contiguous tensor of these extents?  (the stride of an extent-1 axis is never used: anything goes)
inline bool contiguous(const int64_t* shape, const int64_t* strides, int nd) {
  int64_t want = 1;
  for (int d = nd - 1; d >= 0; --d) {
    if (shape[d] != 1 && strides[d] != want) return false;
    want *= shape[d];
  }
  return true;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

// the grid of a kernel that walks `blocks` workgroups' worth of tiles or work items with a grid stride: that many, capped
inline dim3 capped_grid(int64_t blocks) {
  const int64_t cap = 1 << 20;
  return dim3((unsigned)(blocks < cap ? blocks : cap));
}

// f(std::integral_constant<int, V>{}), V = the elements of a 16-byte pack of T where `wide`, else 1: picks the instance of a
// kernel whose template argument is the width of its loads or stores (`decltype(v)::value` inside the generic lambda; nested
// for two widths)
template <typename T, typename F>
void by_pack_width(bool wide, F&& f) {
  if (wide) f(std::integral_constant<int, 16 / (int)sizeof(T)>{});
  else f(std::integral_constant<int, 1>{});
}

// The checks of an entry `who` that reads one contiguous core X [R, I, C] and writes another buffer: dtype, sizes, pointers, the
// strides of X, the index envelope.  `rest`: the entry's other pointers that must not be null, tested with X and `out`;
// `out_name`: what the message calls the output.
inline int core_check(const char* who, int dtype, int64_t R, int64_t I, int64_t C, const void* X, const int64_t* x_strides,
                      const void* out, const char* out_name, bool rest = true) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "%s: bad dtype %d", who, dtype);
  TTR_REQUIRE(R >= 1 && I >= 1 && C >= 1, TTR_E_INVALID, "%s: bad sizes R = %lld, I = %lld, C = %lld", who, (long long)R, (long long)I,
              (long long)C);
  TTR_REQUIRE(X && x_strides && out && rest, TTR_E_INVALID, "%s: null pointer", who);
  TTR_REQUIRE(X != out, TTR_E_INVALID, "%s: X and %s must be different buffers", who, out_name);
  const int64_t xs[3] = {R, I, C};
  TTR_REQUIRE(contiguous(xs, x_strides, 3), TTR_E_UNSUPPORTED, "%s: X must be contiguous", who);
  TTR_REQUIRE((double)R * (double)I * (double)C < 9.0e18 / 64.0, TTR_E_UNSUPPORTED, "%s: core too large", who);
  return TTR_OK;
}

// Y [R, I, C] with element strides (sr, si, 1), rows and slabs that do not overlap; the stride of an extent-1 axis is free
inline int strided_y_check(const char* who, int64_t R, int64_t I, int64_t C, const int64_t* y_strides, int64_t* sr, int64_t* si) {
  *si = I > 1 ? y_strides[1] : C;
  *sr = R > 1 ? y_strides[0] : I * *si;
  TTR_REQUIRE((C == 1 || y_strides[2] == 1) && *si >= C && *sr >= I * *si, TTR_E_UNSUPPORTED,
              "%s: Y needs element strides (sr, si, 1) with si >= C and sr >= I si", who);
  TTR_REQUIRE((double)R * (double)*sr < 9.0e18 / 64.0, TTR_E_UNSUPPORTED, "%s: Y too large", who);
  return TTR_OK;
}

}  // namespace ttr
