// What crosses translation units inside libttround_hip.so and is not in ttr_common.h: the prototypes of the dispatchers the
// extern "C" wrappers call, the knob globals ttr_debug_set_knob writes, and two host helpers.
//
// HOST-ONLY: no __global__ / __device__ code and no template a kernel instantiates.  Including this file therefore cannot
// alter any kernel, which is why it may live outside the set of files bench.py hashes (csrc/*.h and the kernel sources:
// `source_sha` / `KIND_SOURCES`, which tie the counters of profiles/pmc_latest.json to the build they were taken from).
//
// Included by ttr_api.hip, ttr_orth.hip and ttr_vec.hip (the callers) and by ttr_cp.hip and ttr_eigsel.hip (which define
// dispatchers declared here: the compiler checks declaration against definition there).
// FOLLOW-UP, the next time the counters are re-collected: ttr_qr.hip, ttr_sweep.hip, ttr_eigh.hip, ttr_gemm.hip and
// ttr_bjacobi.hip define the rest of these dispatchers and knobs and should include this file too; until then a changed
// signature in one of them shows up at link time only.  (block_sum, which ttr_vec.hip and ttr_orth.hip both carry, moves into
// ttr_common.h on the same occasion.)
#pragma once
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
                  const void* sigma_in = nullptr, int64_t stride_sigma_in = 0);
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
                           const int32_t* rows32 = nullptr);
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
extern int g_eigh_big_occ;
extern int g_sweep_stagger;
extern int g_rank_noise_c;
extern int g_jacobi_live_wave;
extern int g_eigh_small;
extern int g_orth_rounds, g_orth_v2, g_orth_split;   // ttr_orth.hip

inline bool dtype_ok(int dtype) { return dtype == TTR_F32 || dtype == TTR_F64; }

// the census counters of ttr_prof_enable(2) ([2 * TTR_PROF_NKINDS]: flops per kind, then bytes per kind) for kernels that count
// their own work; nullptr unless work_census_on()
double* work_census_dev();

}  // namespace ttr
