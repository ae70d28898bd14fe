/*
 * ttround_hip.h -- C ABI of libttround_hip.so, the MI355X (gfx950) kernels behind
 * tntorch's TT orthogonalisation / rounding hot path.
 *
 * The reference (rballester/tntorch) has NO native layer: the hot path reaches
 * LAPACK/BLAS through torch operators.  Each entry point below therefore replaces
 * one *operator call site* of the reference (file:line given per function), and
 * is what a maintainer would bind with ctypes from tntorch/round.py and
 * tntorch/tensor.py.
 *
 * Conventions
 *   - all matrix pointers are DEVICE pointers; matrices are row-major with an
 *     explicit leading dimension (elements) and a batch stride (elements);
 *   - `dtype` is TTR_F32 or TTR_F64; scalars that select truncation (delta^2)
 *     are passed as double;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream);
 *     every call only enqueues work on that stream, never synchronises, never
 *     allocates: workspaces are caller-provided (sizes from *_workspace_bytes);
 *   - return value: 0 on success, <0 on error (TTR_E_*); ttr_last_error() gives
 *     a thread-local message.
 */
#ifndef TTROUND_HIP_H
#define TTROUND_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTR_F32 0
#define TTR_F64 1

#define TTR_OK 0
#define TTR_E_INVALID (-1)     /* bad argument */
#define TTR_E_UNSUPPORTED (-2) /* shape outside the kernels' envelope */
#define TTR_E_HIP (-3)         /* HIP runtime error */
#define TTR_E_WORKSPACE (-4)   /* workspace too small */

/* scale modes for ttr_gemm epilogues */
#define TTR_SCALE_NONE 0
#define TTR_SCALE_MUL 1
#define TTR_SCALE_DIV 2 /* x / s, and 0 where |s| is below the smallest normal */

/* eigenvalue post-processing modes for ttr_eigh_trunc */
#define TTR_EIG_RAW 0   /* sigma = sqrt(max(w, 0)) */
#define TTR_EIG_REF 1   /* round.py:118-119: w < 0 -> 1e-8 before the sqrt */
#define TTR_EIG_MATCH_DIAG 2 /* like RAW, but NOT sorted: V -> I as G -> diagonal.  Tridiagonal solver: the
                                eigenvector of the r-th largest eigenvalue is written to the column holding
                                the r-th largest diagonal entry of G; Jacobi: eigenpair i stays in column i
                                (rotation angles <= pi/4 never swap).  Building block of the block-Jacobi
                                driver for n above the single-workgroup limit. */

/* ABI version of this header: bumped whenever an exported signature changes (round 2 inserted `gparts` / `stride_gpart` into
   ttr_eigh_trunc = 2; round 3 additions = 3 ... 7, the last one ttr_eigh_top; round 4: 8 = rows32 / skip_zero_rows, 9 = ttr_carry_rows32;
   round 5: 10 = ttr_round_tt, the whole sweep behind one call, + TTR_KNOB_RANK_NOISE_FLOOR; 11 = ttr_qr_factor_expo / ttr_qr_factor_pushed_expo; 12 = ttr_gather_chain; 13 = ttr_maxvol, ttr_gather_step; 14 = ttr_als_normal, ttr_spd_solve, ttr_pinv_finish; 15 = ttr_sparse_keys, ttr_sparse_levels, ttr_sparse_group, ttr_sparse_gram, ttr_sparse_project; 16 = ttr_core_matvec, ttr_hsum_step; 17 = ttr_mode_diff, ttr_laplace_core; ttr_core_convolve, ttr_accept_count / ttr_accept_expand, ttr_mode_scan / ttr_mode_reduce, ttr_pce_design / ttr_pce_predict, ttr_mode_sandwich, ttr_sample_max_rank / ttr_sample_step and ttr_ttm_step / ttr_cpm_step were ADDED under 17: no existing signature changed, and a library without the
   symbols fails at load, in the binding and in build()); so were ttr_gather_grad, ttr_gather_grad_workspace_bytes and
   ttr_gather_grad_stage_rows, and ttr_ttm_grad_input, ttr_ttm_grad_core_slab_rows, ttr_ttm_grad_core_workspace_bytes and
   ttr_ttm_grad_core, and ttr_ttm_lookup_workspace_bytes and ttr_ttm_lookup_step, and ttr_core_compose, and ttr_env_half_apply, and ttr_ritz_parts, ttr_ritz_workspace_bytes, ttr_ritz_gram and
   ttr_ritz_update, and ttr_ttm_lookup_grad_core_slab_rows, ttr_ttm_lookup_grad_core_workspace_bytes, ttr_ttm_lookup_grad_core,
   ttr_ttm_lookup_grad_input_workspace_bytes, ttr_ttm_lookup_grad_input and ttr_segment_sum, and ttr_eigh_trunc_pass and
   ttr_project_flat (+ TTR_KNOB_FLAT_PASS; ttr_eigh_trunc and ttr_project keep their signatures and behaviour), and ttr_cg_parts,
   ttr_cg_workspace_bytes, ttr_cg_dot, ttr_cg_update and ttr_cg_direction.  ttr_version() returns the value the library was built with; the Python
   binding refuses to use a library whose version differs (a stale .so would take misaligned arguments silently). */
#define TTR_ABI_VERSION 17
int ttr_version(void);
const char* ttr_last_error(void);

/* Limits of the LDS/register-resident kernels (queried by the host shim). */
int ttr_qr_max_cols(int dtype);        /* widest panel ttr_qr factors (columns) */
int ttr_eigh_max_n_lds(int dtype);     /* largest n solved out of LDS; above it the solver works out of L2/HBM */
int ttr_eigh_max_n(int dtype);         /* largest n ttr_eigh_trunc accepts (4096 fp32 / 2048 fp64) */

/*
 * C[b] = scale( op(A[b]) * op(B[b]) ),  op(A) is M x K, op(B) is K x N.
 * Replaces: `R @ right_unfolding(core)` tensor.py:1826-1832 (push right),
 *           `M @ M^T` / `M^T @ M` round.py:104-109 (Gram),
 *           `left^T @ M` with the 1/sigma row scaling round.py:163-172 (projection),
 *           `einsum("ijk,kl")` tensor.py:2074-2083 (push left, with the sigma column scaling
 *           of round.py:169-172 fused), `M @ left` round.py:175-181.
 * transA/transB: 0 -> the stored matrix is op(X); 1 -> the stored matrix is op(X)^T.
 * rowscale (length M per batch item) / colscale (length N per batch item) may be NULL.
 * MFMA (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64) on LDS-staged tiles.
 * `workspace` (may be NULL) enables split-K for few-tile / very-long-K products
 * (Gram matrices of tall dense unfoldings); size from ttr_gemm_workspace_bytes.
 */
int64_t ttr_gemm_workspace_bytes(int dtype, int64_t M, int64_t N, int64_t K, int64_t batch);
int ttr_gemm(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K,
             const void* A, int64_t lda, int64_t strideA,
             const void* B, int64_t ldb, int64_t strideB,
             void* C, int64_t ldc, int64_t strideC,
             const void* rowscale, int64_t stride_rs, int rowscale_mode,
             const void* colscale, int64_t stride_cs, int colscale_mode,
             int64_t batch, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * C[b] <- beta * C[b] + alpha * op(A[b]) * op(B[b])   (same kernel; C is read only when beta != 0).
 * Building block of the routines that extend the envelope of the kernels above: block Gram-Schmidt
 * projections  W <- W - Q (Q^T W)  of the QR for n > ttr_qr_max_cols (torch.linalg.qr, tensor.py:1816/1853)
 * and the Newton-Schulz step  V <- 1.5 V - 0.5 V (V^T V)  of the large-n eigensolver (round.py:115).
 */
int ttr_gemm_axpby(int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K,
                   const void* A, int64_t lda, int64_t strideA,
                   const void* B, int64_t ldb, int64_t strideB,
                   void* C, int64_t ldc, int64_t strideC,
                   double alpha, double beta,
                   int64_t batch, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Reduced Householder QR of batch tall (or square/wide) matrices: A[b] (m x n) = Q[b] (m x k) R[b] (k x n),
 * k = min(m, n), LAPACK sign convention (geqrf: beta = -sign(alpha)*norm), R upper triangular/trapezoidal.
 * Replaces: torch.linalg.qr at tensor.py:1816 (left_orthogonalize) and tensor.py:1853/1859
 * (right_orthogonalize, on the transposed unfolding).
 * Communication-avoiding TSQR: 256-row blocks held as MFMA accumulator tiles and factored with the blocked
 * compact-WY algorithm (16-column panels, trailing updates on the matrix cores), R factors reduced over a
 * 4-ary tree, Q formed by walking the tree back (pure MFMA).  n <= ttr_qr_max_cols(dtype).
 */
int64_t ttr_qr_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t batch);
int ttr_qr(int dtype, int64_t m, int64_t n, int64_t batch,
           const void* A, int64_t lda, int64_t strideA,
           void* Q, int64_t ldq, int64_t strideQ,
           void* R, int64_t ldr, int64_t strideR,
           void* workspace, int64_t workspace_bytes, void* stream);
/*
 * The same factorisation with TRANSPOSED addressing -- tensor.py:1853-1863 factors the transpose of the right unfolding
 * (`torch.linalg.qr(unfolding.T)`, torch has no RQ) and transposes Q back (1866-1878).  `At` is the n x m row-major
 * matrix whose TRANSPOSE A (m x n) is factored; `Qt` receives Q^T (k x m row-major, ldqt >= m); R as for ttr_qr.  The
 * kernels read / write through (row, column) strides, nothing is copied.
 */
int ttr_qr_t(int dtype, int64_t m, int64_t n, int64_t batch,
             const void* At, int64_t ldat, int64_t strideAt,
             void* Qt, int64_t ldqt, int64_t strideQt,
             void* R, int64_t ldr, int64_t strideR,
             void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The two halves of ttr_qr, for callers that fuse work into the formation of Q:
 *   ttr_qr_factor  factors A (TSQR tree of blocked compact-WY Householder blocks on MFMA), writes R (k x n) and
 *                  leaves the reflectors / T factors in `workspace` (which must stay alive and untouched);
 *   ttr_qr_apply   forms Out[b] (m x kcols) = Q[b] * C[b], C (k x kcols, kcols <= k) -- C == NULL means the
 *                  identity, i.e. the first kcols columns of Q.  round_tt uses it to produce core * (U sigma)
 *                  directly (the "push left" einsum of tensor.py:2081-2083) without ever materialising Q.
 */
int ttr_qr_factor(int dtype, int64_t m, int64_t n, int64_t batch,
                  const void* A, int64_t lda, int64_t strideA,
                  void* R, int64_t ldr, int64_t strideR,
                  void* workspace, int64_t workspace_bytes, void* stream);
int ttr_qr_apply(int dtype, int64_t m, int64_t n, int64_t batch,
                 void* workspace, int64_t workspace_bytes,
                 const void* C, int64_t ldc, int64_t strideC, int64_t kcols,
                 void* Out, int64_t ldo, int64_t strideO, void* stream);
/*
 * ttr_qr_factor with the sweep's power-of-two normalisation folded in (ABI 11; fp32 only): R comes back as R 2^-e, e the binary
 * exponent of the largest entry of the TOP block of the TSQR tree (max |entry| of what is returned times 2^e lies within a factor
 * sqrt(rows) of 1: O(1), exact scaling), and e is ADDED to expo_acc[item] (device int32 [batch]).  The left-to-right loop of a
 * rounding (tensor.py:1905-1906) multiplies the norms of all cores into the last R: 64^8 randn cores reach 2^72 in fp32, sums and
 * products more; the sweep therefore keeps every R at O(1) and gives the exponents back to the first core at the end (exact).
 * Rounds 1 - 4 did that with one ttr_pow2_normalize launch per core; the factor kernel already scales its block by a power of two
 * (its fp32 range guard) and here simply does not scale R back.  Reflectors and T factors are scale invariant: ttr_qr_apply on
 * the same workspace is unchanged.  ttr_qr_factor_pushed_expo: the same for the fused push.
 */
int ttr_qr_factor_expo(int dtype, int64_t m, int64_t n, int64_t batch,
                       const void* A, int64_t lda, int64_t strideA,
                       void* R, int64_t ldr, int64_t strideR,
                       void* workspace, int64_t workspace_bytes, int32_t* expo_acc, void* stream);

/*
 * Fused "push right + QR" of the left-to-right sweep (tensor.py:1823-1832 followed by tensor.py:1816 of the next
 * core): factors the (k*I) x n left unfolding of  P[kk, i, c] = sum_r0 Rm[kk, r0] * core[r0, i, c]  without ever
 * writing P.  Rm is the R factor of the previous core (k x Rin, k, Rin <= 64), `core` the next core, contiguous
 * [Rin, I, n].  The TSQR row blocks are chosen as {(kk, i): i = 4b .. 4b+3}, so every wave forms its own 64 x n
 * slice Rm * core[:, i, :] on the matrix cores straight into the accumulator tiles it then factors.
 * ttr_qr_apply_pushed is the matching ttr_qr_apply (Out rows in the natural order kk*I + i).  Needs k*I >= n.
 */
int64_t ttr_qr_pushed_workspace_bytes(int dtype, int64_t I, int64_t n, int64_t batch);
int ttr_qr_factor_pushed(int dtype, int64_t k, int64_t Rin, int64_t I, int64_t n, int64_t batch,
                         const void* Rm, int64_t ldrm, int64_t strideRm,
                         const void* core, int64_t stride_core,
                         void* R, int64_t ldr, int64_t strideR,
                         void* workspace, int64_t workspace_bytes, void* stream);
int ttr_qr_factor_pushed_expo(int dtype, int64_t k, int64_t Rin, int64_t I, int64_t n, int64_t batch,
                              const void* Rm, int64_t ldrm, int64_t strideRm,
                              const void* core, int64_t stride_core,
                              void* R, int64_t ldr, int64_t strideR,
                              void* workspace, int64_t workspace_bytes, int32_t* expo_acc, void* stream);
/*
 * The same fused push + factorisation for the middle core of a TT SUM a + b (tensor.py:445-668): the next core is the
 * block-diagonal blockdiag(a_core [ra][I][ca], b_core [rb][I][cb]) of tensor.py's `__add__`, which is never
 * materialised -- the kernel reads the two blocks where they lie (column tiles inside one block only walk that block's
 * rows: half the multiply-adds of the padded core for equal ranks).  Rm is k x (ra + rb); workspace size and the
 * implicit Q (ttr_qr_apply_pushed) are those of ttr_qr_factor_pushed with n = ca + cb.  This is the "add, then round"
 * fusion of tools.reduce (tools.py:460-512).
 */
int ttr_qr_factor_pushed_sum(int dtype, int64_t k, int64_t I, int64_t batch,
                             const void* Rm, int64_t ldrm, int64_t strideRm,
                             const void* core_a, int64_t ra, int64_t ca, int64_t stride_a,
                             const void* core_b, int64_t rb, int64_t cb, int64_t stride_b,
                             void* R, int64_t ldr, int64_t strideR,
                             void* workspace, int64_t workspace_bytes, void* stream);
int ttr_qr_apply_pushed(int dtype, int64_t k, int64_t I, int64_t n, int64_t batch,
                        void* workspace, int64_t workspace_bytes,
                        const void* C, int64_t ldc, int64_t strideC, int64_t kcols,
                        void* Out, int64_t ldo, int64_t strideO, int skip_zero_rows, void* stream);
/* `skip_zero_rows` != 0: for the items whose factorisation packed its rows (TTR_KNOB_QR_PACK; flags at
 * ttr_qr_pushed_flag_offset) the exactly-zero rows kk >= 32 of Out are NOT written -- a third of the kernel's HBM traffic; the
 * caller then reads Out only through kernels that take the item's flag (`rows32` of ttr_rowgram / ttr_rotgram / ttr_project). */
/*
 * ttr_qr_apply_pushed that ALSO emits the row Gram matrix of its output, G = M M^T of the k x (I*kcols) right unfolding M of
 * Out (round.py:104-109: what the truncation of the next bond computes first), accumulated from the output tiles while
 * they are still in registers -- the right-to-left sweep reads the new carry twice instead of three times.
 * G: [batch][parts][k][k] contiguous split partials (both triangles), parts = ttr_qr_apply_pushed_gram_parts(...); the
 * eigensolver sums them on load (ttr_eigh_trunc's gparts).  parts == 0: this shape is not covered (fp32, k = 64, kcols = 32,
 * I a multiple of 8 are), call ttr_qr_apply_pushed + ttr_rowgram instead.  ldo must equal kcols.
 * Requires TTR_KNOB_QR_PACK == 0 from before the factorisation until after this call (the epilogue walks the unpacked row map
 * of the level-0 blocks); with the knob != 0 the call returns TTR_E_UNSUPPORTED instead of a Gram matrix with unwritten partials.
 */
int64_t ttr_qr_apply_pushed_gram_parts(int dtype, int64_t k, int64_t I, int64_t n, int64_t kcols);
int ttr_qr_apply_pushed_gram(int dtype, int64_t k, int64_t I, int64_t n, int64_t batch,
                             void* workspace, int64_t workspace_bytes,
                             const void* C, int64_t ldc, int64_t strideC, int64_t kcols,
                             void* Out, int64_t ldo, int64_t strideO, void* G, void* stream);

/*
 * Symmetric eigen-decomposition + the rank rule of truncated_svd, batched, on device.
 * Input  G[b]  (n x n symmetric, e.g. a Gram matrix).
 * Output V[b]  (n x n): eigenvectors as COLUMNS, sorted by DEcreasing sigma,
 *        sigma[b] (n): sqrt of the (clamped) eigenvalues, decreasing,
 *        info[b]  (int32): the selected rank r >= 1, or 0 if sigma_max < 1e-13 (round.py:137-145 zero guard).
 * Rank rule (round.py:147-158): drop the longest tail with sum(sigma^2) <= delta2, then
 * r = max(1, min(rmax, n - tail)); with use_delta == 0 (batch mode, round.py:149-150) r = max(1, min(rmax, n)).
 * Replaces: torch.linalg.eigh round.py:115, the clamp/sqrt/argsort of round.py:118-135 and the rank
 * selection round.py:147-158 (and, in the two-pass 'svd' algorithm, torch.linalg.svd round.py:96).
 * Parallel cyclic two-sided Jacobi; out of LDS for n <= ttr_eigh_max_n_lds(dtype), else out of `workspace`.
 * Rotations are skipped when |G_pq| <= sqrt(n)*eps*sqrt(G_pp*G_qq) (relative criterion: high relative
 * accuracy on graded, accurately formed Gram matrices -- pass 2 of the 'svd' algorithm).  abs_floor = 1
 * additionally skips |G_pq| <= sqrt(n)*eps*max|G_ii| (for a plain Gram matrix, whose entries are only
 * accurate to eps*||G||).  abs_floor = 2 selects, for n <= 64, the tridiagonal solver instead (Householder
 * reduction + implicit-shift QL, two waves per matrix, absolute accuracy O(eps*||G||) like LAPACK steqr):
 * ~10x fewer flops, used for the first pass / 'eig'; larger n falls back to Jacobi with abs_floor = 1.
 * abs_floor = TTR_SOLVER_JACOBI_LIVE (pass 2 of the two-pass 'svd' truncation): purely relative rotation test among
 * the LIVE indices; indices with G_ii <= (n eps)^2 max G_ii (the numerical null space of the input) are frozen.  Every
 * live direction gets the accuracy of a backward-stable SVD (LAPACK gesdd class, round.py:96) whatever its sigma.
 * `sweeps` (optional, [batch]) receives the number of sweeps (Jacobi) / QL iterations used.
 * eig_mode = TTR_EIG_MATCH_DIAG: see above (sigma[b] then follows V's column order; info as usual).
 * TTR_EIG_RAW / TTR_EIG_REF clamp negative eigenvalues: G is taken to be positive semi-definite up to rounding (a Gram matrix).  The
 * tridiagonal solver uses that for a 64 x 64 matrix whose diagonal is exactly zero from index 32 on (zero rows / columns: the
 * carry of a bond whose QR packed its rows): it is solved as its leading 32 x 32 block, V[b] = blockdiag(V11, I), sigma[b][32:] = 0.
 * PRECONDITION of RAW / REF therefore: G is a Gram matrix (PSD up to rounding: G_ii = 0 implies a zero row).  A general symmetric
 * matrix -- e.g. [[0, 1], [1, 0]] padded to 64 x 64 -- must be passed with TTR_EIG_MATCH_DIAG, which neither clamps nor shrinks.
 * The input may be given as `gparts` partial matrices (split-K partials of a Gram kernel, `stride_gpart` elements
 * apart): G[b] = sum_p G[b * strideG + p * stride_gpart + ...]; gparts = 1 for a plain matrix.
 */
#define TTR_SOLVER_JACOBI_REL 0
#define TTR_SOLVER_JACOBI_ABS 1
#define TTR_SOLVER_TRIDIAG 2
#define TTR_SOLVER_JACOBI_LIVE 3
int64_t ttr_eigh_workspace_bytes(int dtype, int64_t n, int64_t batch);
int ttr_eigh_trunc(int dtype, int64_t n, int64_t batch,
                   const void* G, int64_t ldg, int64_t strideG, int64_t gparts, int64_t stride_gpart,
                   void* V, int64_t ldv, int64_t strideV,
                   void* sigma, int64_t stride_sigma,
                   int32_t* info,
                   int eig_mode, int use_delta, double delta2, const double* delta2_dev, int64_t rmax,
                   int abs_floor, int32_t* sweeps,
                   const int32_t* skip_items, const void* sigma_in, int64_t stride_sigma_in,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* `skip_items` / `sigma_in` (optional; Jacobi solvers): pass-through items of the two-pass truncation, see
 * ttr_spectrum_flat below.
 * `delta2_dev` (optional, device pointer to ONE double): the bound delta^2 of the rank rule taken from device memory instead
 * of `delta2` -- tensor.py:2039-2051 computes delta from the norm of the last core and reads it back (`.item()`); an
 * eps-mode sweep that keeps it on the device enqueues every bond without a host synchronisation. */
/* Pass 2 of the two-pass truncation for a caller that hands `skip_items` to ttr_project_flat as well: ttr_eigh_trunc, except that
 * V of a pass-through item is NOT written (nobody reads the identity; 4 n^2 bytes per item).  Its sigma (= sigma_in: ttr_orth_fixup
 * reads it), info and sweeps are written as usual.  TTR_KNOB_FLAT_PASS = 0: ttr_eigh_trunc itself. */
int ttr_eigh_trunc_pass(int dtype, int64_t n, int64_t batch,
                        const void* G, int64_t ldg, int64_t strideG, int64_t gparts, int64_t stride_gpart,
                        void* V, int64_t ldv, int64_t strideV,
                        void* sigma, int64_t stride_sigma,
                        int32_t* info,
                        int eig_mode, int use_delta, double delta2, const double* delta2_dev, int64_t rmax,
                        int abs_floor, int32_t* sweeps,
                        const int32_t* skip_items, const void* sigma_in, int64_t stride_sigma_in,
                        void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Pass 1 of a batch-mode bond with 40 <= n <= 64 rows and a rank cap r <= 32, r < n (ttr_eigh_top_ok): round.py:96, 147-158 with
 * the rank fixed to rmax never looks below sigma_r.  Two waves per matrix: Householder tridiagonalisation + forward formation of Q as
 * in ttr_eigh_trunc's tridiagonal solver, then -- instead of the QL iteration over the whole spectrum -- Sturm-count multisection
 * for lambda_1..r, one twisted factorisation per eigenvalue (MRRR getvec), Z^T Z -> two Newton-Schulz steps for orthonormality,
 * V[:, :r] = Q Z (Z^T Z)^{-1/2} on MFMA.
 * The kernel decides PER ITEM whether that result can be trusted: the kept spectrum must be flat (sigma_r >= thr sigma_1 > 0, the
 * criterion of ttr_spectrum_flat) and free of close pairs (neighbouring kept eigenvalues >= 512 eps lambda_1 apart: inverse
 * iteration on isolated eigenvalues needs no reorthogonalisation beyond the Newton-Schulz polish).  flat[b] = 1: V[b][:, :r],
 * sigma[b][:r] = sqrt(lambda) (descending), the rest of V[b] / sigma[b] zero, info[b] = r.  flat[b] = 0 or 2: the item fell through to
 * the QL phase of the same launch and carries the full decomposition, exactly what ttr_eigh_trunc(eig_mode = TTR_EIG_RAW,
 * abs_floor = TTR_SOLVER_TRIDIAG, rmax = n) returns; 2 when its sigma pass ttr_spectrum_flat's batch-mode test (sigma_r >= thr
 * sigma_1 > 0: declined for a close pair only), so that flat[b] != 0 IS the pass-through flag of the bond's second pass -- no
 * ttr_spectrum_flat launch, no merge of two flag arrays (round 4; two launches per bond on a latency-bound chain).  `flat` is optional.
 * A 64 x 64 matrix whose diagonal is exactly zero from index 32 on (the Gram matrix of a carry with zero rows 32.., a bond whose QR
 * packed its rows) is solved as its leading 32 x 32 block (G must be a Gram matrix: G_ii = 0 => row i = 0): flat[b] = 1 as above,
 * otherwise V[b] = blockdiag(V11, I), sigma[b][32:] = 0.
 */
int ttr_eigh_top_ok(int64_t n, int64_t r);
int ttr_eigh_top(int dtype, int64_t n, int64_t batch,
                 const void* G, int64_t ldg, int64_t strideG, int64_t gparts, int64_t stride_gpart,
                 void* V, int64_t ldv, int64_t strideV,
                 void* sigma, int64_t stride_sigma,
                 int32_t* info, int64_t r, double thr, int32_t* flat, int need_all, void* stream);
/* `need_all` != 0 (ABI 10; the first pass of an eps-mode bond, whose rank rule needs every singular value): the top-r path only
 * takes items of which it computes EVERY eigenpair -- r >= the item's live size, i.e. the zero-tail (32 x 32) problems of a packed
 * bond under a cap r >= 32; all other items get the full QL decomposition of the same launch.  sigma / V are then complete for
 * every item (structural zeros / unit vectors beyond a shrunk block), exactly as ttr_eigh_trunc(TTR_EIG_RAW, TTR_SOLVER_TRIDIAG)
 * returns them, and `flat` is not meaningful (the caller runs ttr_spectrum_flat with use_delta). */

/*
 * Selected eigenpairs of symmetric matrices with 64 < n <= ttr_eigsel_max_n() (1024): the k <= 64 LARGEST eigenvalues and their
 * eigenvectors -- torch.linalg.eigh / svd of round.py:96, 115 on the Gram matrix of a dense TT-SVD bond when only the top of the
 * spectrum is looked at (batch mode with a rank cap far below n: BASELINE config C3, n = 256, rmax = 8).  LAPACK syevx class:
 *   ttr_tridiag       A[b] (n x n symmetric, leading dimension lda, DESTROYED) = Q T Q^T by Householder reflectors, one
 *                     workgroup per matrix; d[b][n], e[b][n] (e[i] couples i and i + 1, e[n-1] = 0), tau[b][n]; reflector k is
 *                     left in row k of A (columns k+1 .., leading 1 stored).  `workspace` (optional, ttr_tridiag_workspace_bytes):
 *                     with it, few (<= 4) big (n >= 512) matrices are reduced by 2 n - 1 launches that spread every step's pass
 *                     over the whole chip instead of one workgroup per matrix
 *   ttr_tri_eigsel    lam[b][k] = the k largest eigenvalues of T (descending; Sturm-count multisection) and Z[b][n][k] their
 *                     unit eigenvectors (twisted factorisation: close eigenvalues leave them only NEARLY orthogonal -- the host
 *                     shim orthonormalises Z with ttr_qr and falls back when a column collapses);
 *                     scratch: ttr_eigsel_scratch_bytes(dtype, n, batch)
 *   ttr_tridiag_back  Z[b] <- Q[b] Z[b] (in place), A / tau as left by ttr_tridiag
 */
int ttr_eigsel_max_n(void);
int64_t ttr_eigsel_scratch_bytes(int dtype, int64_t n, int64_t batch);
int64_t ttr_tridiag_workspace_bytes(int dtype, int64_t n, int64_t batch);
int ttr_tridiag(int dtype, int64_t n, int64_t batch, void* A, int64_t lda, int64_t strideA, void* d, void* e, void* tau,
                void* workspace, int64_t workspace_bytes, void* stream);
int ttr_tri_eigsel(int dtype, int64_t n, int64_t batch, int64_t k, const void* d, const void* e, void* lam, void* Z, void* scratch,
                   int64_t scratch_bytes, void* stream);
int ttr_tridiag_back(int dtype, int64_t n, int64_t batch, int64_t k, const void* A, int64_t lda, int64_t strideA, const void* tau,
                     void* Z, void* stream);

/*
 * Block-Jacobi driver for symmetric eigenproblems above the single-workgroup limit -- torch.linalg.eigh / svd of
 * round.py:96, 115 on the n = I r Gram matrices of a dense TT-SVD (BASELINE configs C1: n = 1024, C3: n = 256).
 * G[item] (n x n, n = 2 b npairs, b <= 32) and the accumulated eigenvector matrix V[item] are updated IN PLACE, one
 * round = ttr_bj_solve + ttr_bj_apply with the round's pairing `pair_tab` (device int32 [npairs][2]: block indices of
 * every pair; over nbk - 1 rounds of a round-robin tournament every two blocks meet once = one sweep):
 *   ttr_bj_solve    W[item * npairs + p] (w x w, w = 2 b) = eigenvectors of the pair's diagonal problem
 *                   [[G_ii, G_ij], [G_ji, G_jj]], diagonal-matched column order (W -> I as the problem -> diagonal);
 *                   `scratch`: ttr_bj_scratch_bytes(...).
 *   ttr_bj_apply    G[P, Q] <- W_p^T G[P, Q] W_q for all pairs of pairs, V[:, Q] <- V[:, Q] W_q; with `offsq` (device
 *                   double [items], optional) the squared off-diagonal entries of the updated G are added to offsq[item].
 *   ttr_bj_control  once per sweep: sets ctrl[0] = 1 ("converged") when no pair problem of the sweep rotated anything
 *                   (relative != 0) or when max_item sqrt(offsq[item]) / gnorm[item] <= tol or stagnates (relative == 0;
 *                   gnorm = ||G[item]||_F of the input, element type of `dtype`); resets ctrl[1] and offsq.
 * ctrl: device int32 [4] = {converged, pair problems that rotated in the current sweep, sweeps performed, unused}, zeroed
 * by the caller; state: device double [items + 1] = offsq followed by the previous sweep's ratio (initialise to -1).
 * Once ctrl[0] is set every later ttr_bj_* launch returns at its first instruction: the caller enqueues the maximum
 * number of sweeps and never reads anything back.
 */
int64_t ttr_bj_scratch_bytes(int dtype, int64_t b, int64_t npairs, int64_t items);
int ttr_bj_solve(int dtype, int64_t b, int64_t npairs, int64_t items,
                 const void* G, int64_t ldg, int64_t strideG, const int32_t* pair_tab,
                 void* W, void* scratch, int32_t* ctrl, void* stream);
int ttr_bj_apply(int dtype, int64_t b, int64_t npairs, int64_t items,
                 void* G, int64_t ldg, int64_t strideG, void* V, int64_t ldv, int64_t strideV,
                 const int32_t* pair_tab, const void* W, const int32_t* ctrl, double* offsq, void* stream);
int ttr_bj_control(int dtype, int64_t items, int32_t* ctrl, double* state, const void* gnorm, int relative, double tol,
                   void* stream);

/*
 * CP-ALS building blocks (tn.Tensor(X, ranks_cp=R), tensor.py:279-394; BASELINE config C4).
 * ttr_krp_contract:  out[p, q, r] = sum_j T[p, j, q, r] * B[j, r]   (T contiguous [P, J, Q, R], B is J x R with
 * leading dimension ldb, out contiguous [P, Q, R]).  One step of a fused MTTKRP: the reference materialises the
 * Khatri-Rao matrix (`torch.einsum("ir,jr->ijr")` chain, tensor.py:328-334) and a permuted copy of the dense
 * unfolding (tensor.py:336) and multiplies them (tensor.py:338); here the tensor is first contracted with one
 * factor by ttr_gemm (X read once) and the remaining modes are folded in with this kernel (Q = 1: trailing mode,
 * P = 1: leading mode), each reading its input exactly once.
 * ttr_hadamard: out[i] = a[i] * b[i] -- the Gram Hadamard product `prod *= grams[m]` (tensor.py:331).
 */
int ttr_krp_contract(int dtype, int64_t P, int64_t J, int64_t Q, int64_t R,
                     const void* T, const void* B, int64_t ldb, void* out, void* stream);
int ttr_hadamard(int dtype, int64_t count, const void* a, const void* b, void* out, void* stream);

/*
 * Slice-wise Kronecker product of two TT cores (the Hadamard product of two tensor trains multiplies the ranks):
 *   out[b, r1*S1 + s1, i, r2*S2 + s2] = a[b, r1, i, r2] * c[b, s1, i, s2],   a [B, R1, I, R2], c [B, S1, I, S2] contiguous.
 * Replaces: `_core_kron` tensor.py:2309-2320 (called from `Tensor.__mul__`, tensor.py:687-773), the producer of the
 * rank-inflated trains the rounding sweeps exist for.
 */
int ttr_core_kron(int dtype, int64_t batch, int64_t R1, int64_t S1, int64_t I, int64_t R2, int64_t S2,
                  const void* a, const void* c, void* out, void* stream);

/*
 * out[b] = sqrt(sum(x[b]^2)) over `count` contiguous elements (accumulated in double, stored in dtype).
 * Replaces: torch.norm(cores[-1]) tensor.py:2039-2051 and torch.norm(M) round.py:80.
 */
int ttr_norm(int dtype, int64_t count, int64_t batch, const void* x, int64_t stride_x, void* out, void* stream);

/*
 * out[b][i][j] = in[b][i][j] * s[b][j]   (mode TTR_SCALE_MUL)  or  / s[b][j]  (TTR_SCALE_DIV).
 * Replaces: `left * svd[1][:rank]` round.py:169-172 and the 1/sigma column scaling round.py:175.
 */
int ttr_scale_cols(int dtype, int64_t rows, int64_t cols, int64_t batch,
                   const void* in, int64_t ldi, int64_t stride_in,
                   const void* s, int64_t stride_s, int mode,
                   void* out, int64_t ldo, int64_t stride_out, void* stream);
/* x[b][:, j] <- 0 for j >= keep[b], in place (keep: device int32 [batch], e.g. ttr_eigh_trunc's info).  The device-side
 * form of `left = vectors[..., :rank]` (round.py:160-161) for a sweep that computes every bond at its rank cap and reads the
 * selected ranks back once, at the end (at most one host synchronisation per round_tt).
 * keep[b] >= cols leaves item b untouched; keep[b] < 0 is clamped to 0 (the whole item is zeroed, nothing outside its
 * rows x cols window is written). */
int ttr_mask_cols(int dtype, int64_t rows, int64_t cols, int64_t batch, void* x, int64_t ldx, int64_t stride_x,
                  const int32_t* keep, void* stream);


/*
 * Fused kernels of the right-to-left truncation sweep: the (R <= 64) x n right unfolding M of a core is streamed once,
 * 16 columns per wave and step, every intermediate stays in MFMA accumulator registers.
 *   ttr_rowgram   G = M M^T                                           replaces `M @ M^T` round.py:104-109
 *   ttr_rotgram   G = (V1^T M)(V1^T M)^T  (V1: R x R)                 pass 2 of the two-pass 'svd' truncation (round.py:96):
 *                 the Gram matrix of the rows ROTATED by the pass-1 eigenvectors, formed from the rotated data (small
 *                 rows from small numbers) without ever writing the rotated matrix
 *   ttr_project   right = diag(1/sigma) U^T M (ro x n),  left = U diag(sigma) (R x ro, optional),  U = V1 V2[:, :ro]
 *                 (V1 = NULL: U = V2[:, :ro]); scale_right = 0: right = U^T M, left = U        replaces round.py:163-172
 * G is written as `nparts` split-K partial matrices per item ([batch][nparts][R][R], contiguous; nparts from
 * ttr_sweep_gram_parts); ttr_eigh_trunc sums them on load.
 */
int64_t ttr_sweep_gram_parts(int64_t n, int64_t batch);
int ttr_rowgram(int dtype, int64_t R, int64_t n, int64_t batch, const void* M, int64_t ldm, int64_t strideM,
                void* G, int64_t nparts, const int32_t* rows32, void* stream);
/* `rows32` (ttr_rowgram, ttr_project; optional device int32 [batch]): != 0 -> rows 32.. of this item's M are exactly zero and are
 * not loaded (half the reads of an HBM-bound kernel).  Source: the flags a packed ttr_qr_factor_pushed leaves in its workspace at
 * byte offset ttr_qr_pushed_flag_offset (TTR_KNOB_QR_PACK: the carry ttr_qr_apply_pushed produces from such a factorisation has
 * zero rows kk >= 32). */
int64_t ttr_qr_pushed_flag_offset(int dtype, int64_t I, int64_t n, int64_t batch);
/* The same flags for a carry that no fused push follows -- the LAST core of the left-to-right sweep, tensor.py:2053-2056's first
 * truncation: flag[b] = 1 when rows 32.. of the 64 x cols matrix R[b] hold at most (c eps)^2 of ||R[b]||_F^2 (c =
 * TTR_KNOB_QR_RANK_SKIP; the packing test of ttr_qr_factor_pushed).  Since round 5 the sweep (tntorch_amd/_hipops.py, ttr_round_tt)
 * calls it ON THE CARRY ITSELF, M = R_{N-2} x (last core) as a 64 x (I r) matrix, not on the R factor: what ttr_rowgram /
 * ttr_rotgram / ttr_project then treat as zero (`rows32`) is below c eps ||M||_F whatever the last core's condition number is --
 * but it is DROPPED energy, not a structural zero: rows 32.. of M are non-zero in memory.  The eps-mode rank rule accounts for it
 * through the noise floor (TTR_KNOB_RANK_NOISE_FLOOR, default 1: sigma[32..] count as eps sigma_0 and ttr_spectrum_flat tests the
 * whole spectrum with its robustness margin E = 64 n eps sigma_0^2 >= (c eps)^2 ||M||^2); with the floor switched off the 32
 * trailing values are exact zeros to the rule and a tolerance below c eps (fp64, eps < 2e-15) may select fewer directions than
 * LAPACK's (ABI 9). */
int ttr_carry_rows32(int dtype, int64_t cols, int64_t batch, const void* R, int64_t ldr, int64_t strideR, int32_t* flag,
                     void* stream);
int ttr_rotgram(int dtype, int64_t R, int64_t n, int64_t batch, const void* M, int64_t ldm, int64_t strideM,
                const void* V1, int64_t ldv1, int64_t strideV1, void* G, int64_t nparts, const int32_t* skip,
                const int32_t* rows32, void* stream);
/*
 * When is the second pass needed?  The first Gram matrix G = M M^T carries sigma_i^2 with an ABSOLUTE error of c eps sigma_1^2
 * (c: a small constant of the fp32 accumulation), i.e. sigma_i and the unit norm of row i of `right` to c eps (sigma_1 /
 * sigma_i)^2 / 2: the second pass exists for kept singular values far below sigma_1.  When the `keep` kept ones lie within
 * a factor 1 / thr of each other (the host shim uses thr = 1/8; measured with the kernels' accumulation order emulated
 * on the CPU: right-orthonormality 8e-7 / relative sigma error 4e-7 after one pass against 4e-7 / 2e-7 after two at
 * sigma_keep = sigma_1 / 8), one pass already is in the accuracy class of the two.  ttr_spectrum_flat writes
 * flat[b] = (sigma[b][r - 1] >= thr * sigma[b][0] > 0) from pass 1's sigma (sorted decreasing), r = the rank the item will get:
 *   use_delta = 0 or delta^2 = 0 (batch mode, round.py:149-150, or no eps): r = keep = min(rank cap, n);
 *   use_delta = 1 (delta2, or *delta2_dev when given): r from the tail-energy rule of round.py:147-158 on pass 1's sigma, and the
 *     item only qualifies when that decision is robust against pass 1's absolute error E = 64 n eps sigma_1^2 of a tail energy:
 *     tail(r) <= delta^2 - E and tail(r - 1) > delta^2 + E (rank cap binding, r = keep: only the latter) -- pass 2 would select
 *     the same rank.  (fp32 with eps = 1e-4: E exceeds delta^2, nothing qualifies; fp64 trains do.)
 * ttr_rotgram skips items with skip[b] != 0 (their G is not written) and ttr_eigh_trunc passes them through
 * (`skip_items`: V = I, sigma = sigma_in, rank rule as usual on sigma_in).  The sweep calls ttr_eigh_trunc_pass and
 * ttr_project_flat instead, which leave the identity out (TTR_KNOB_FLAT_PASS).
 */
int ttr_spectrum_flat(int dtype, int64_t n, int64_t batch, const void* sigma, int64_t stride_sigma, int64_t keep, double thr,
                      int use_delta, double delta2, const double* delta2_dev, int32_t* flat, const int32_t* rows32, void* stream);
/* `rows32` (optional, ABI 10): the flags ttr_rowgram took for this bond -- sigma[32..] of a flagged item are structural zeros (exact
 * in either pass), so in eps mode the rule's cut of them is certain and only the 32 computed values are tested for robustness:
 * a rank-deficient train (t = g + g) rounded through the reference's NON-batch call skips its second Gram pass like a batch. */
int ttr_project(int dtype, int64_t R, int64_t n, int64_t ro, int64_t batch,
                const void* M, int64_t ldm, int64_t strideM,
                const void* V1, int64_t ldv1, int64_t strideV1,
                const void* V2, int64_t ldv2, int64_t strideV2,
                const void* sigma, int64_t stride_sigma, int scale_right,
                void* right, int64_t ldr, int64_t strideR,
                void* left, int64_t ldl, int64_t strideL, const int32_t* rows32, void* stream);
/* ttr_project with the pass-through flags of the two-pass truncation.  `flat` (optional device int32 [batch]: the `skip` of
 * ttr_rotgram, the `skip_items` of ttr_eigh_trunc_pass) and `sigma1` (pass 1's sigma, `stride_sigma1` elements per item): an item
 * with flat[b] != 0 has V2 = I and sigma = sigma1 by construction, so neither V2 nor sigma is loaded and no V1 V2 is formed for it --
 * U = V1[:, :ro], scales from sigma1: the bits of the product with the identity.  Items with flat[b] == 0, and every item when
 * `flat` or `V1` is NULL or TTR_KNOB_FLAT_PASS is 0, are ttr_project's. */
int ttr_project_flat(int dtype, int64_t R, int64_t n, int64_t ro, int64_t batch,
                     const void* M, int64_t ldm, int64_t strideM,
                     const void* V1, int64_t ldv1, int64_t strideV1,
                     const void* V2, int64_t ldv2, int64_t strideV2,
                     const void* sigma, int64_t stride_sigma, int scale_right,
                     void* right, int64_t ldr, int64_t strideR,
                     void* left, int64_t ldl, int64_t strideL, const int32_t* rows32,
                     const int32_t* flat, const void* sigma1, int64_t stride_sigma1, void* stream);

/*
 * The same fused kernels for TALL matrices (rows x n, n <= 64, row-major): the unfoldings a dense right-to-left TT-SVD
 * truncates first -- prod(I_1..I_{N-1}) rows, I_N columns, the whole input tensor in bytes (tensor.py:401-408 via
 * round.py:101-135 with the Gram matrix on the short side).  The contraction runs over the rows, 16 per wave and step.
 *   ttr_colgram     G = M^T M   (V1 = NULL)   or   G = (M V1)^T (M V1): the rotated matrix is never written
 *                   (`workspace`: split-K partials, size from ttr_colgram_workspace_bytes; G is the reduced n x n matrix)
 *   ttr_colproject  left = M U [diag(1/sigma)] (rows x ro),  right = [diag(sigma)] U^T (ro x n),  U = V1 V2[:, :ro]
 *                   (left_ortho = 1: the scalings in brackets, round.py:173-178; 0: round.py:179-182)
 * A 'svd' truncation of such an unfolding therefore reads it three times and writes only ro / n of its size.
 */
int64_t ttr_colgram_workspace_bytes(int dtype, int64_t rows, int64_t n, int64_t batch);
int ttr_colgram(int dtype, int64_t rows, int64_t n, int64_t batch, const void* M, int64_t ldm, int64_t strideM,
                const void* V1, int64_t ldv1, int64_t strideV1, void* G, void* workspace, int64_t workspace_bytes,
                const int32_t* skip /* optional [batch], as ttr_rotgram's */, void* stream);
int ttr_colproject(int dtype, int64_t rows, int64_t n, int64_t ro, int64_t batch,
                   const void* M, int64_t ldm, int64_t strideM,
                   const void* V1, int64_t ldv1, int64_t strideV1,
                   const void* V2, int64_t ldv2, int64_t strideV2,
                   const void* sigma, int64_t stride_sigma, int left_ortho,
                   void* left, int64_t ldl, int64_t strideL,
                   void* right, int64_t ldr, int64_t strideR, void* stream);

/*
 * Exact power-of-two normalisation, one launch: e[b] = binary exponent of ||x[b]|| (0 for a zero / non-finite norm),
 * out[b] = x[b] * 2^-e[b], and, when `expo_acc` is given, expo_acc[b] += e[b].  (`out` may alias `x`; out = NULL:
 * exponents only.)
 * Replaces the LAPACK-internal rescaling the reference relies on (torch.linalg.qr / svd are scale safe,
 * tensor.py:1816, round.py:96): the fp32 sweep keeps every R factor at O(1) and returns the summed exponent to core 0.
 */
int ttr_pow2_normalize(int dtype, int64_t count, int64_t batch, const void* x, int64_t stride_x,
                       void* out, int64_t stride_out, int32_t* e_out, int32_t* expo_acc, void* stream);

/*
 * out[b][i] = x[b][i] * scale[b * stride_scale] * 2^(expo_sign * expo[b])   (scale and/or expo may be NULL;
 * stride_scale = 0 broadcasts one scalar).  Replaces scalar multiplications of cores (tensor.py:687-773 with a
 * scalar operand) and gives the exponents of ttr_pow2_normalize back.
 */
int ttr_scale_batch(int dtype, int64_t count, int64_t batch, const void* x, int64_t stride_x,
                    const void* scale, int64_t stride_scale, const int32_t* expo, int expo_sign,
                    void* out, int64_t stride_out, void* stream);

/*
 * Orthonormal completion of the numerically null directions a truncation keeps.  X[b] holds `r` vectors of length `n`
 * (vector i, element k at X[b * strideX + i * vec_stride + k * elem_stride]); sigma[b] are the singular values,
 * decreasing.  Vectors i < r with sigma_i <= dead_rel * sigma_0 carry rounding noise only (their sigma is below the
 * resolution of the input): they are re-orthogonalised against all previous vectors (modified Gram-Schmidt, twice;
 * a vector that vanishes is replaced by a hashed pseudo-random one) and normalised, so that the factor is orthonormal
 * to working accuracy like the V of a LAPACK SVD (round.py:96), while the product left * right changes by
 * O(dead_rel * sigma_0) only.  Items without such vectors exit immediately (the normal case).
 */
int64_t ttr_orth_fixup_workspace_bytes(int dtype, int64_t r, int64_t n, int64_t batch, int64_t elem_stride);
int ttr_orth_fixup(int dtype, int64_t r, int64_t n, int64_t batch, void* X, int64_t vec_stride, int64_t elem_stride,
                   int64_t strideX, const void* sigma, int64_t stride_sigma, double dead_rel, const int32_t* rank_dev,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* `workspace` (ABI 10; may be NULL): with ttr_orth_fixup_workspace_bytes(...) > 0 bytes of it, a LARGE batch (>=
 * TTR_KNOB_ORTH_SPLIT items, default 2048; vectors as rows, <= 64 of them) runs its first two rounds as three launches each -- the
 * Gram matrix by ttr_rowgram's kernel (split-K partials summed in double), the coefficients, the streamed product X_dead <- W X
 * (which, for <= 32 vectors, also leaves the second round's Gram matrix: that round has two launches) --
 * instead of one workgroup per item, and ONE launch of the single-workgroup kernel finishes the items that need more (remainders
 * that collapsed and were replaced: rare).  Same rounds, same semantics (a vector with non-finite entries counts as the zero
 * vector), ~2x the HBM rate.  Without a workspace (or below the threshold) the single-launch kernel does everything. */
/* `rank_dev` (optional, device int32 [batch]): only the first min(r, rank_dev[b]) vectors of item b are looked at -- a sweep
 * that computes its factors at the rank cap and cuts them to the selected rank later does not complete vectors it drops. */

/*
 * The WHOLE rounding of a batch of tensor trains in ONE call (ABI 10): the left-to-right orthogonalisation loop of
 * tensor.py:1905-1906 (tensor.py:1816-1832 per core) followed by the right-to-left truncation loop of tensor.py:2053-2083
 * (round.py:52-187 per bond) -- the two Python loops of `Tensor.round_tt` (tensor.py:2008-2083).  The entry enqueues, on
 * `stream`, the same kernels in the same order as the per-kernel entries above would be called by a host loop (results are
 * bit-identical to that loop); it allocates nothing, synchronises nothing and reads nothing back.
 *
 *   shapes     host int64 [3 N]: (r0, I, r1) of every input core; cores_in[mu] = contiguous [batch][r0][I][r1] on the device
 *   rcap       host int64 [N - 1] or NULL: rank cap of bond mu = 1 .. N-1 at index mu - 1 (>= 2^31 - 1: none, round.py:83-84)
 *   algorithm  TTR_ALG_SVD (two Gram passes: the accuracy class of gesdd, round.py:96) / TTR_ALG_EIG (round.py:101-135)
 *   eps_mode   0 = batch semantics (round.py:149-150: every bond is cut at its cap, eps is ignored; any batch);
 *              1 = the reference's NON-batch rule for ONE train (batch == 1): delta = eps / max(1, sqrt(N - 1)) ||last core||
 *              (tensor.py:2039-2051) is formed ON THE DEVICE, every bond is computed at its cap, the rank the rule of
 *              round.py:147-158 selects is written to ranks_dev[mu - 1] and the cores are ZERO beyond the selected ranks: the
 *              caller reads ranks_dev once, after the call, and slices (ranks_dev[i] == 0: the zero guard of round.py:137-145)
 *   flat_thr   items whose kept singular values lie within a factor 1 / flat_thr skip the second Gram pass (ttr_spectrum_flat;
 *              0 = never); use_eigh_top != 0: batch-mode first passes through ttr_eigh_top where ttr_eigh_top_ok
 *   cores_out  cores_out[mu] = contiguous [batch][q_mu][I][q_{mu+1}], q_0 = r0 of core 0, q_N = r1 of the last core,
 *              q_mu = max(1, min(rcap[mu - 1], rows of bond mu)) -- the ranks batch mode produces (fixed by the shapes)
 *   zero_flag_dev  optional device-ACCESSIBLE int32 [1] (eps_mode 0): receives the largest rank-rule result of the FIRST truncation
 *              over the batch; 0 = every item hit the zero guard (round.py:137-141) and the caller returns the rank-1 zero train.
 *              Written by a one-workgroup kernel right after that truncation (with a system-scope fence): device memory, or --
 *              what tntorch_amd passes since round 6 -- a pinned host word the caller initialises to a sentinel and polls, so
 *              that it need not wait for the rest of the sweep before it returns.  eps_mode 1 (round 6): when given, an int32
 *              [N - 1] device-accessible array that receives a COPY of ranks_dev as soon as the last bond is decided (N - 1 <= 64),
 *              i.e. before the last projection and the first core are formed -- the same polling pattern for the reference's
 *              non-batch call
 *   workspace  ttr_round_tt_workspace_bytes(...) bytes, caller-owned; the call may be repeated with the same workspace once the
 *              previous one has completed on the stream
 * Envelope: every TT rank <= ttr_qr_max_cols, every core inside the fused push (k, Rin <= 64, k I >= n), every bond a
 * <= 64-row matrix with at least as many columns.  ttr_round_tt_workspace_bytes returns TTR_E_UNSUPPORTED (< 0) outside it:
 * the caller then runs its own loop over the per-kernel entries.
 */
#define TTR_ALG_SVD 0
#define TTR_ALG_EIG 1
int64_t ttr_round_tt_workspace_bytes(int dtype, int64_t N, const int64_t* shapes, const int64_t* rcap, int64_t batch,
                                     int eps_mode);
int ttr_round_tt(int dtype, int64_t N, const int64_t* shapes, int64_t batch, const void* const* cores_in, const int64_t* rcap,
                 int algorithm, int eps_mode, double eps, double flat_thr, int use_eigh_top, void* const* cores_out,
                 int32_t* ranks_dev, int32_t* zero_flag_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* Per-kernel device timing (HIP events on `stream`), used by bench.py for the roofline line. */
#define TTR_PROF_GEMM 0
#define TTR_PROF_QR_FACTOR 1
#define TTR_PROF_QR_APPLY 2
#define TTR_PROF_EIGH 3
#define TTR_PROF_MISC 4
#define TTR_PROF_ROTGRAM 5
#define TTR_PROF_PROJECT 6
#define TTR_PROF_ROWGRAM 7
#define TTR_PROF_NKINDS 8
/* Diagnostics: when set to a device buffer of >= 64 int64, block (0,0) of every level-0 QR factor launch writes
 * its s_memtime stamps at phase boundaries there.  NULL disables. */
int ttr_debug_set_qr_stamps(void* device_buffer);
/* Diagnostics / A-B measurements: select kernel variants at run time (process-wide, not thread safe).
 *   TTR_KNOB_QR_PANEL  1 = the 8-wave QR blocks factor / apply their panel columns in pairs (two reflectors per step,
 *                      v_permlane-swap reductions; default), 0 = one reflector at a time (round-1 kernel). */
#define TTR_KNOB_QR_PANEL 0
/*   TTR_KNOB_BJ_INNER_SWEEPS  cyclic sweeps ttr_bj_solve spends on every pair problem (0 = until the pair problem has
 *                      converged; default 1: the outer iteration converges with inexact inner solves -- W is a product of
 *                      rotations either way -- and a round costs a fraction) */
#define TTR_KNOB_BJ_INNER_SWEEPS 1
/*   TTR_KNOB_GEMM_BIG  1 (default) = fp32 products with both output dimensions >= 128 run on the 128 x 128-tile kernel
 *                      (symmetric products: upper-triangle tiles only); 0 = the 64 x 64-tile kernel everywhere (A/B runs) */
#define TTR_KNOB_GEMM_BIG 2
/*   TTR_KNOB_QR_STAMP_BX / _BY  which level-0 block of ttr_qr_factor* writes the cycle stamps of ttr_debug_set_qr_stamps
 *                      (block index within the matrix / batch item; default (0, 0), which starts with the first wave of
 *                      workgroups -- a block in the middle of the grid shows the steady state) */
#define TTR_KNOB_QR_STAMP_BX 3
#define TTR_KNOB_QR_STAMP_BY 4
/*   TTR_KNOB_QR_F64_NW4  1 = fp64 TSQR trees consist of 256-row (4-wave) blocks only -- two blocks per CU; 0 (default) = the
 *                      512-row (8-wave) blocks of the fp32 path (132 KB of LDS in fp64: one block per CU; measured 17 %
 *                      faster on config C2 all the same).  Bit 1 (value 2 / 3): the same for fp32 (round 4's A/B on the metric
 *                      workload).  Set it BEFORE any workspace is sized (an A/B switch). */
#define TTR_KNOB_QR_F64_NW4 5
/*   TTR_KNOB_QR_RANK_SKIP  c (default 8): the 8-wave QR blocks do not factor a panel whose remaining part is below c eps of the
 *                      block's Frobenius norm (rank-inflated trains: H = I, tau = 0; ttr_qr_apply skips trailing identity
 *                      panels); 0 = every panel is factored (A/B). */
#define TTR_KNOB_QR_RANK_SKIP 6
/*   TTR_KNOB_QR_PACK  3 (default) = level 0 of a fused push (ttr_qr_factor_pushed) whose R factor has rows 32 .. 63 below
 *                      c eps of its norm (c: TTR_KNOB_QR_RANK_SKIP) drops the pushed rows (kk >= 32, i) as zeros and packs two
 *                      mode indices per wave: blocks b < nb / 2 do all the work, the others write a zero R and return, and the
 *                      launch is block-major (all working blocks first); decided per item on the device,
 *                      ttr_qr_apply_pushed follows the per-item flag the factor kernel leaves in the workspace.  1 / 2 = the
 *                      item-major variants (measured without gain: the dispatcher stalls on alternating long / short
 *                      workgroups); 0 = never (required for ttr_qr_apply_pushed_gram, whose epilogue assumes the unpacked map). */
#define TTR_KNOB_QR_PACK 7
/*   (8 = TTR_KNOB_EIGH_SMALL, below)
 *   TTR_KNOB_RANK_NOISE_FLOOR  c (default 1 since round 6; 0 = off): the rank rule of round.py:147-158 (eps mode: ttr_eigh_trunc
 *                      with use_delta, ttr_spectrum_flat) sees every singular value at no less than c eps sigma_0.  Background: the
 *                      zero-tail eigenproblems of a rank-deficient bond (t = g + g) return EXACT zeros for the null directions, which
 *                      the rule would cut at any delta >= 0; LAPACK's gesdd -- the reference -- returns rounding noise of order
 *                      eps sigma_0 there, so `round_tt(rmax=48)` (eps = 1e-14 by default) on a numerically rank-32 fp32 train keeps
 *                      the cap.  c = 1 reproduces the reference's outcome (fp32: the cap; fp64: eps^2 < 1e-28, still cut);
 *                      TTR_STRICT_RANKS=0 in the environment of tntorch_amd sets 0. */
#define TTR_KNOB_RANK_NOISE_FLOOR 9
/*   TTR_KNOB_ORTH_ROUNDS  (default 4) upper bound on the rounds of ttr_orth_fixup's block variant (diagnostics: what a round costs;
 *                      fewer than the data needs leaves the completed directions short of orthonormal).  In census mode
 *                      (ttr_prof_enable(2)) the MISC counters receive flops += rounds executed, bytes += items with dead directions. */
#define TTR_KNOB_ORTH_ROUNDS 10
/*   TTR_KNOB_JACOBI_LIVE_WAVE  1 = ttr_eigh_trunc with TTR_SOLVER_JACOBI_LIVE on n <= 64 runs ONE wave per matrix (no cross-wave
 *                      barrier in the round loop): measured SLOWER (1.25 vs 0.80 ms per launch of 2048 matrices, round 5);
 *                      0 (default) = the four-wave kernel. */
#define TTR_KNOB_JACOBI_LIVE_WAVE 11
/*   TTR_KNOB_ORTH_V2  1 = ttr_orth_fixup's block variant for <= 32 vectors runs the round-5 inner loops (wide LDS operand
 *                      reads with a permuted K order, dead tile rows only, chunk columns split over the four waves); 0 = round 4's (A/B);
 *                      2 (default) = 1 + the three-launch rounds of a large batch with <= 32 vectors skip the second round's Gram launch:
 *                      the first round's product launch leaves the Gram matrix of the vectors as it wrote them (A/B against 1). */
#define TTR_KNOB_ORTH_V2 12
/*   TTR_KNOB_QR_INTERLEAVE  1 (default) = the block-major launches of TTR_KNOB_QR_PACK = 3 (ttr_qr_factor_pushed level 0,
 *                      ttr_qr_apply_pushed level 0) order the workgroups of each half item by item (an item's working blocks follow
 *                      each other), so that resident workgroups differ in the address bits their block index fixes -- HBM channel
 *                      spreading; 0 = all items' block 0, then all items' block 1, ... (round 4; A/B). */
#define TTR_KNOB_QR_INTERLEAVE 13
/*   TTR_KNOB_SWEEP_STAGGER  the fused <= 64-row sweep kernels walk an item's columns starting at step (item index mod steps) and
 *                      wrap around, so that resident workgroups do not read the same column offsets (= the same HBM channels:
 *                      every item's rows are ldm elements apart and aligned alike) at the same time.  1 (default) = ttr_project only
 *                      (independent columns: bit-identical results); 2 = ttr_rowgram / ttr_rotgram as well (their sums are then
 *                      accumulated in an item-dependent order); 0 = in order (A/B). */
#define TTR_KNOB_SWEEP_STAGGER 14
/*   TTR_KNOB_ORTH_SPLIT  batch size (per launch) from which ttr_orth_fixup, given a workspace, runs its rounds as three launches
 *                      (default 2048; 0 = always the single-launch kernel): 13 % on a 4096-train step whose kept directions mostly
 *                      lie below the resolution (sigma ~ 2^-j), nothing measurable on one without dead directions at that size
 *                      (the launches that exit at once cost 0.3 - 2 % at 1024 items: hence the threshold). */
#define TTR_KNOB_ORTH_SPLIT 15
/*   TTR_KNOB_QR_STAGGER  k (default 0 = off; round 6, A/B): workgroups 256 .. 511 of a fused push + factor launch (the second
 *                      resident block of every CU under round-robin dispatch) start k x 1024 cycles late, so that a CU's two blocks
 *                      alternate their HBM phase (the push) and their panel chain instead of running them side by side. */
#define TTR_KNOB_QR_STAGGER 16
/*   TTR_KNOB_QR_PACK_PRE  1 (default; round 6) = the row-packing decision of a fused push + factor launch (TTR_KNOB_QR_PACK) is
 *                      taken by a one-wave-per-item kernel AHEAD of the launch and read by its blocks: an absorbed block returns at
 *                      once instead of staging Rm first (9 k cycles each, 16384 of them at the tail of every level-0 launch of the
 *                      metric), its partner writes the zero R block and taus for it; 0 = every block derives the decision from Rm
 *                      itself (round 5; A/B).  + 2: level 1 of a packed item treats the absorbed leaves' (exactly zero) rows as ordinary
 *                      rows, in ttr_qr_factor_pushed and ttr_qr_apply_pushed alike (A/B; default: the factor kernel runs its panel
 *                      chain over the live half only and the apply kernel's waves on the zero rows load, multiply and store
 *                      nothing; bit-identical results either way). */
#define TTR_KNOB_QR_PACK_PRE 17
/*   TTR_KNOB_EIGH_BIG_OCC  0 (default) / 3 / 2 = waves per SIMD the 64-row instance of ttr_eigh_top is built for in fp32 launches of
 *                      >= 1024 matrices (0: four waves, 128 registers, 106 spilled; 3: 168 registers; 2: 256 registers, none
 *                      spilled); bit-identical results (A/B, round 6). */
#define TTR_KNOB_EIGH_BIG_OCC 18
/*   TTR_KNOB_EIGH_SMALL  1 = ttr_eigh_top and the tridiagonal solver of ttr_eigh_trunc (TTR_EIG_RAW / REF) on 64 x 64
 *                      matrices first run the 32-row instance of their kernel over the zero-tail items (Gram matrices of packed
 *                      bonds) and then the 64-row one over the rest; 0 = one launch, the 64-row instance shrinks such items
 *                      itself (A/B); 2 (default) = 1, and fp32 ttr_eigh_top launches of >= 1024 matrices use the lean build of the
 *                      32-row instance: pivots of the twisted factorisation in LDS, 108 VGPRs under the 128-register cap of four
 *                      waves per SIMD, no scratch (1: 208 VGPRs, two waves) -- same results bit for bit; 3 = the 128-register
 *                      cap, which is that same build. */
#define TTR_KNOB_EIGH_SMALL 8
/*   TTR_KNOB_SWEEP_LEAN  1 (default) = fp32 launches of ttr_rowgram and ttr_project (kept rank <= 32) on 64-row matrices with a
 *                      `rows32` pointer and >= 256 items run twice: a lean build of the kernel for the flagged items (rows 0 .. 31
 *                      only: 3 Gram tiles with three slabs requested ahead / 8 K steps with the U fragments in registers; 8
 *                      workgroups per CU instead of 4) and the generic build for the rest, each returning at once for the other's
 *                      items -- same results bit for bit; 0 = the generic build alone (A/B). */
#define TTR_KNOB_SWEEP_LEAN 19
/*   TTR_KNOB_QR_PAIR4  1 (default) = level 1 of the packed items of a fused push + factor launch of >= 256 items (fp32; the items
 *                      whose rows 256 .. 511 are zero, see TTR_KNOB_QR_PACK_PRE) is factored by the FOUR-wave instance of the pair
 *                      kernel: the 256 live rows as a 256-thread block, two column pairs per wave, four blocks -- four panel chains
 *                      -- per CU where the 8-wave instance for four live row groups has two; same arithmetic in the same order,
 *                      bit-identical results, same workspace layout; 0 = that 8-wave instance (A/B).  + 2: plain fp32 matrices of
 *                      <= 256 rows and more than 32 columns (ttr_qr_factor) run on the four-wave pair instance too instead of the
 *                      single-step kernel: rank-revealing pair steps, so the last bits of R differ (tests, and the A/B of the
 *                      first core of a sweep); the workspace layout is the 4-wave one either way. */
#define TTR_KNOB_QR_PAIR4 20
/*   TTR_KNOB_FLAT_PASS  1 (default) = the pass-through items of the two-pass truncation (flat kept spectrum, ttr_spectrum_flat)
 *                      skip the identity round trip: ttr_eigh_trunc_pass does not write their V, and ttr_project_flat takes
 *                      U = V1[:, :ro] and 1 / sigma from pass 1's sigma for them without loading V2 or sigma or forming V1 V2.  The
 *                      product with an exact identity adds exact zeros to one exact term: same results bit for bit.  0 =
 *                      ttr_eigh_trunc_pass writes V = I as ttr_eigh_trunc does and ttr_project_flat ignores its flags (A/B). */
#define TTR_KNOB_FLAT_PASS 21
int ttr_debug_set_knob(int knob, int value);
int ttr_prof_enable(int on);   /* 0 = off, 1 = per-kind device times, 2 = times + executed-work census (ttr_prof_collect_work) */
/* Synchronises the recorded events; fills total milliseconds and launch counts per kind; resets. */
int ttr_prof_collect(double* ms, int64_t* launches);
/* Census mode (ttr_prof_enable(2); ABI 10): flops / bytes the instrumented launches EXECUTED since the last collect, per kind --
 * read off the same device-side decisions the kernels took (zero taus of rank-skipped / absorbed QR panels, packing flags,
 * `rows32` and pass-through flags), by tiny kernels enqueued outside the timed scopes.  Instrumented: qr_factor, qr_apply (flops),
 * rowgram, rotgram, project (flops and bytes), gemm (flops and bytes of the dense product).  Synchronises the device; resets. */
int ttr_prof_collect_work(double* flops, double* bytes);


/*
 * Batched TT point evaluation (ABI 12): the index-array block of tensor.py:1019-1434 (`t[idx_matrix]`, `t[:, [..], [..]]`).
 * For a contiguous block of `nmodes` cores G_n (batched [B, r_n, I_n, r_{n+1}], element strides core_strides[4n .. 4n+3] =
 * batch, r, I, r') and one index column per mode (P entries, element stride idx_strides[n], int32 (idx_dtype 0) or int64 (1),
 * negative entries wrap as in torch):
 *     out[b, :, p, :] = G_0[b][:, i_0[p], :] @ G_1[b][:, i_1[p], :] @ ... @ G_{nmodes-1}[b][:, i_{nmodes-1}[p], :]
 * (r_0 x r_nmodes), written at out + b*stride_ob + i*stride_or + p*stride_op + j*stride_oc -- the reference's [r_a, P, r_b] core.
 * Replaces: the per-mode `einsum("iaj,jak->iak")` chain over gathered slices, tensor.py:1357-1378.
 * `ranks` (nmodes + 1 entries), `sizes`, `cores`, `core_strides`, `idx`, `idx_strides` are HOST arrays (of device pointers).
 * Points are grouped by index value with a device counting sort per mode, and each slice is multiplied against the 64 running-
 * product rows of a tile that share it; P <= direct_max_points (< 0: library default, 1024) skips the sort (one tile per point).
 * Both paths give bitwise identical values, and a point's value does not depend on the other points of the call.
 * Every index is validated on the device first: the int32 word at `oob_flag` (device) is set to 1 when an index lies outside
 * [-I_n, I_n), and to 0 otherwise; when set, nothing else is written.  The caller reads the word after the call.
 * Ranks <= 512, batch <= 65535.  P == 0 clears the word and returns; `out` and the index columns may then be NULL.
 */
int64_t ttr_gather_chain_workspace_bytes(int dtype, int64_t nmodes, const int64_t* ranks, const int64_t* sizes, int64_t P,
                                         int64_t batch);
int ttr_gather_chain(int dtype, int64_t nmodes, int64_t batch, int64_t P, const int64_t* ranks, const int64_t* sizes,
                     const void* const* cores, const int64_t* core_strides, int idx_dtype, const void* const* idx,
                     const int64_t* idx_strides, void* out, int64_t stride_ob, int64_t stride_or, int64_t stride_op,
                     int64_t stride_oc, int64_t direct_max_points, void* oob_flag, void* workspace, int64_t workspace_bytes,
                     void* stream);

/*
 * One gather step with a row map on its input (ABI 13; the interface update of TT-cross, cross.py:400-448):
 *     Y[p, :] = X[xrow[p], :] @ G[:, idx[p], :]          p = 0 .. P-1
 * X [rows_x, r] (row stride ldx, unit column stride), G [r, I, rn] at element strides gr, gi, gj, Y [P, rn] (row stride ldy).
 * `xrow` (int64, device, may be NULL: X[p]) and `idx` (int64, device) are validated on the device: the int32 word at
 * `oob_flag` is set to 1 when an entry is out of range (then nothing else is written), else 0.  `idx` may be negative
 * (-I <= idx < I, wrapped as in torch); `xrow` may not (0 <= xrow < rows_x).  The per-element FMA order is
 * ttr_gather_chain's.  Ranks <= 512.  No workspace, no host synchronisation.
 */
int ttr_gather_step(int dtype, int64_t P, int64_t rows_x, int64_t r, int64_t rn, int64_t I, const void* X, int64_t ldx,
                    const void* xrow, const void* G, int64_t gr, int64_t gi, int64_t gj, const void* idx, void* Y, int64_t ldy,
                    void* oob_flag, void* stream);

/*
 * Maximum-volume rows (ABI 13; maxvol.py:115-170, py_maxvol with top_k_index = -1) of a batch of tall matrices
 * A [batch, N, r] (row-major, item stride stride_ab), N > r, r <= 128:
 *   index [batch, r] (int64, device): the chosen rows;  C [batch, N, r] (item stride stride_cb) = A A[index]^-1.
 * Initial rows from LU with partial pivoting (getrf's pivots, ties to the first position), then Sherman-Morrison-Woodbury swaps
 * while max |C| > tol (tol < 1 counts as 1) and fewer than max_iters swaps were made; the pivot of a swap is the first maximum
 * of |C^T| in row-major order (the reference's divmod(abs(C).argmax(), N)).  C is solved fresh from the final rows.
 * `status` (optional, device int32 [batch, 2]): done flag and number of swaps per item.  Every launch is independent of the host:
 * nothing is read back.  Workspace: ttr_maxvol_workspace_bytes.  Items are independent: a batch gives bitwise the per-item result.
 */
int64_t ttr_maxvol_workspace_bytes(int dtype, int64_t N, int64_t r, int64_t batch);
int ttr_maxvol(int dtype, int64_t batch, int64_t N, int64_t r, const void* A, int64_t stride_ab, double tol, int64_t max_iters,
               void* index, void* C, int64_t stride_cb, void* status, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * TT completion by ALS (ABI 14; interpolation.py:9-119, `optimize_core`): the per-slice least-squares update of core mu, ranks
 * r0 x r1, K = r0 r1 <= 1024.  A sample p of slice i contributes the Khatri-Rao row k_p = L_p (x) R_p, k_p[a r1 + b] = L_p[a] R_p[b]
 * (L [P, r0] the left interfaces, R [P, r1] the right ones, both row-major with leading dimensions ldl / ldr), so the solution
 * x_i reshapes directly to core[:, i, :].  (The reference orders its design columns (b, a) and reshapes them as (a, b): its cores
 * with two ranks > 1 come out scrambled.  These entries compute the true minimiser.)
 *
 * ttr_als_normal replaces the per-slice `torch.where` / Khatri-Rao product / lstsq of the reference with the normal equations,
 * accumulated per TASK t (a run perm[task_begin[t] .. task_end[t]) of the samples of one slice; the caller splits long slices
 * into several tasks, so skewed data does not serialise on one workgroup):
 *   Gp[t] (K x K, contiguous) = sum_p w_p^2 k_p k_p^T,   hp[t] (K) = sum_p w_p^2 y_p k_p      (w NULL: w_p = 1)
 * on v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 (true fp64 / fp32 inputs), the rows k_p formed in registers from LDS-staged
 * L / R rows: the P x K design matrix is never stored.  The lower-triangle 16 x 16 tiles are spread over
 * ttr_als_normal_groups(r0, r1) workgroups per task; Gp is written exactly symmetric.  An empty task writes zeros.
 * No workspace, no host synchronisation.
 */
int64_t ttr_als_normal_groups(int64_t r0, int64_t r1);
int ttr_als_normal(int dtype, int64_t ntasks, int64_t r0, int64_t r1, const void* L, int64_t ldl, const void* R, int64_t ldr,
                   const void* w, const void* y, const void* perm, const void* task_begin, const void* task_end, void* Gp,
                   void* hp, void* stream);
/*
 * Batched SPD solve of the summed systems (replaces the reference's per-slice lstsq): item i (0 <= i < n_items) is the sum of
 * the partials Gp / hp [part_off[i] - part_base, part_off[i + 1] - part_base) (part_off: int64, device).  One workgroup per item,
 * right-looking Cholesky out of LDS when (K^2 + K) elements fit in 60 KiB, else in place in Gsum / hsum (global memory).
 * status[i] (int32) = 1: solved, x_i written to X[i s_item + (k / inner) s_a + (k % inner) s_b], k = 0 .. K-1;
 *                   = 0: a pivot fell to K eps max(diag G_i) or below, or counts[i] < K (`counts`, optional int64 [n_items]:
 *                     the item's number of samples -- fewer than K make it singular whatever the rounding).  X is
 *                     not written; Gsum[i] (K x K) / hsum[i] (K) receive the summed system for the minimum-norm fallback:
 *                     ttr_eigh_trunc(Gsum, TTR_EIG_RAW, skip_items = status, Jacobi), t = V^T hsum (ttr_gemm), then
 * ttr_pinv_finish: for the items with status 0, x_i = V diag(lambda+) t with lambda = sigma^2, lambda+ = 1 / lambda above
 * K eps lambda_max and 0 at or below it (gelsd's minimum-norm solution of the normal equations).  No host synchronisation.
 */
int ttr_spd_solve(int dtype, int64_t n_items, int64_t K, const void* Gp, const void* hp, const void* part_off, int64_t part_base,
                  void* X, int64_t inner, int64_t s_item, int64_t s_a, int64_t s_b, void* Gsum, void* hsum, void* status,
                  const void* counts, void* stream);
int ttr_pinv_finish(int dtype, int64_t n_items, int64_t K, const void* V, const void* sigma, const void* t, const void* status,
                    void* X, int64_t inner, int64_t s_item, int64_t s_a, int64_t s_b, void* stream);

/*
 * Gradient of one core from the samples (added under ABI 17; the backward of the differentiable point evaluation t[X], the step
 * torch autograd takes in the reference's tn.optimize loops: tensor.py:1357-1378 under autograd).  With the left interfaces
 * L [P, r0] and the right interfaces R [P, r1] of a mode (row-major, leading dimensions ldl >= r0 / ldr >= r1; R seeded with the
 * incoming gradient),
 *     dG[:, i, :] = sum over the tasks of slice i, in task order, of  sum_{p in task} L[p]^T R[p]
 * dG a contiguous [r0, I, r1] tensor.  Tasks as for ttr_als_normal: task t is the run perm[task_begin[t] .. task_end[t]) of the
 * samples of ONE slice (perm: int64 sample numbers grouped by slice), task_off (int64 [I + 1]) gives the tasks of each slice.
 * A slice without tasks and an empty task give exact zeros.
 * One workgroup per (task, 64 x 64 tile of (a, b)); the sample axis is the K dimension of v_mfma_f32_16x16x4_f32 /
 * v_mfma_f64_16x16x4_f64 (true fp32 / fp64 inputs), the rows gathered through perm into LDS, ttr_gather_grad_stage_rows(dtype, r0,
 * r1) samples per pass; ranks and runs that are no multiple of the tile are padded with zeros in LDS.  No atomics: a slice with one
 * task writes dG directly, a slice with several writes partials ([r0, r1] per task) to `workspace`
 * (ttr_gather_grad_workspace_bytes) and a second launch sums them in task order: the same inputs give the same bits.
 * Ranks <= 512 (TTR_E_UNSUPPORTED above).  ntasks == 0 writes zeros.  No host synchronisation.
 */
int64_t ttr_gather_grad_stage_rows(int dtype, int64_t r0, int64_t r1);
int64_t ttr_gather_grad_workspace_bytes(int dtype, int64_t ntasks, int64_t r0, int64_t r1);
int ttr_gather_grad(int dtype, int64_t I, int64_t ntasks, int64_t r0, int64_t r1, const void* L, int64_t ldl, const void* R,
                    int64_t ldr, const void* perm, const void* task_begin, const void* task_end, const void* task_off, void* dG,
                    void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Sparse TT-SVD from samples (ABI 15; interpolation.py:122-218, `sparse_tt_svd`): the TT-SVD of the tensor that holds P samples
 * y at the integer positions X [P, N] and zeros elsewhere.  The reference scatters the samples of every step into a dense
 * nrows x ncols matrix D (`sparse_covariance`, `full_times_sparse`; ncols = the number of distinct index suffixes, ~P for sparse
 * data) and multiplies it; these entries work on the samples themselves and never build D.
 *
 * Canonical order (once per decomposition).  ttr_sparse_keys validates X (int64, element strides sx0 / sx1) against `shape`
 * (device int64 [N]): the int32 word at `flag` is set to 0, then bit 0 is set when an index lies outside [0, shape[n]); when it
 * is set nothing else is written.  Otherwise key[p] = ((x_N I_{N-1} + x_{N-1}) ...) I_1 + x_1 (x_N the major key; the caller
 * guarantees prod(shape) < 2^63; key = NULL: validation only).  The caller sorts the keys (any device sort) and passes the
 * sorting permutation (int32 [P]; P < 2^31) to ttr_sparse_levels: lev[p] (int32) = the deepest mode, 1-based, in which sorted sample p differs from
 * sorted sample p - 1 (N for p = 0); a repeated position gets 0 and sets bit 1 of `flag` (which this entry does not clear;
 * with bit 0 set it writes nothing).  In this order the columns of EVERY step n -- the distinct suffixes x_{n+1..N} -- are
 * contiguous runs that start where lev >= n + 1, and inside a run the entries ascend in x_n: nothing is sorted again.
 *
 * The unfolding of a step is a block table: column c owns the blocks colptr[c] .. colptr[c + 1) (int32 [C + 1]), block b sits
 * at mode index blk_i[b] (int32, ascending inside a column, each at most once) and carries r values V[b * ldv + a] -- rows
 * a * I + blk_i[b] of column c of D.  (Step 1: the blocks are the sorted samples, r = 1; after a step, its columns with the q
 * projected values are the next step's blocks.)
 *
 * ttr_sparse_gram   G (n x n, n = r I, leading dimension ldg) = D D^T:
 *                       G[a I + i][b I + j] = sum over the columns c that hold both i and j of V_ci[a] V_cj[b].
 *                   `blkcol` (int32 [nb]): the column of every block; `ilist` (int32 [nb]): the blocks grouped by mode index,
 *                   ascending block number within a group (a stable sort of blk_i); `iptr` (int32 [I + 1]): the groups.
 *                   A workgroup owns one i, a range of j >= i and a tile of (a, b); it walks the blocks of i in list order and,
 *                   for each, the partner blocks of that block's column inside its j range: sum_c m_c^2 r^2 / 2 multiply-adds
 *                   (m_c = blocks of column c).  Every element is one thread's fma chain in ascending column order; a long i
 *                   list is split into ttr_sparse_gram_parts(...) parts whose partial matrices (in `workspace`,
 *                   ttr_sparse_gram_workspace_bytes) are summed in part order; j < i is mirrored.  No floating-point atomics:
 *                   G is exactly symmetric and bit-identical from run to run; rows / columns of a mode index that never occurs
 *                   are exact zeros.  r I <= ttr_eigh_max_n(dtype).
 * ttr_sparse_project W[c * ldw + k] = sum over the blocks b of column c, ascending, and a = 0 .. r-1 of
 *                       V[b][a] * U[(a I + blk_i[b]) * su_row + k * su_col],    k = 0 .. q-1
 *                   i.e. W[c] = sum_b V_b @ core[:, blk_i[b], :] with core = U[:, :q] viewed as [r, I, q]: the gather step of
 *                   ttr_gather_step fused with the segmented sum over a column, `core` read from the eigenvector matrix where
 *                   it lies.  W [C, q] is the next step's V.
 * ttr_sparse_group  the blocks grouped by mode index, for ttr_sparse_gram: ilist (int32 [nb]) = a STABLE counting sort of the block
 *                   numbers by blk_i (chunk histograms in LDS, one scan, a ranked scatter: the device sort idiom of
 *                   ttr_gather_chain), iptr (int32 [I + 1]) = the group offsets.  I <= 4096.  Workspace:
 *                   ttr_sparse_group_workspace_bytes.  Entries of blk_i outside [0, I) are left out.
 * All index arrays are bounds-checked where they are used as addresses (out-of-range entries are skipped).
 */
int ttr_sparse_keys(int64_t P, int64_t N, const void* X, int64_t sx0, int64_t sx1, const void* shape, void* key, void* flag,
                    void* stream);
int ttr_sparse_levels(int64_t P, int64_t N, const void* X, int64_t sx0, int64_t sx1, const void* perm, void* lev, void* flag,
                      void* stream);
int64_t ttr_sparse_group_workspace_bytes(int64_t nb, int64_t I);
int ttr_sparse_group(int64_t nb, int64_t I, const void* blk_i, void* ilist, void* iptr, void* workspace, int64_t workspace_bytes,
                     void* stream);
int64_t ttr_sparse_gram_parts(int dtype, int64_t r, int64_t I, int64_t nb);
int64_t ttr_sparse_gram_workspace_bytes(int dtype, int64_t r, int64_t I, int64_t nb);
int ttr_sparse_gram(int dtype, int64_t r, int64_t I, int64_t nb, int64_t C, const void* colptr, const void* blk_i,
                    const void* blkcol, const void* ilist, const void* iptr, const void* V, int64_t ldv, void* G, int64_t ldg,
                    void* workspace, int64_t workspace_bytes, void* stream);
int ttr_sparse_project(int dtype, int64_t r, int64_t I, int64_t q, int64_t nb, int64_t C, const void* colptr, const void* blk_i,
                       const void* V, int64_t ldv, const void* U, int64_t su_row, int64_t su_col, void* W, int64_t ldw,
                       void* stream);

/*
 * Contractions of the TT moment family (ABI 16; metrics.py:345-455, `hadamard_sum`), both on v_mfma_f32_16x16x4_f32 /
 * v_mfma_f64_16x16x4_f64 (true fp32 / fp64 inputs), both without host synchronisation.
 *
 * ttr_core_matvec   the product of a TT-matrix core with a TT-vector core (metrics.py:434-445, `einsum("ijkl,akbc->iajblc")`
 *                   with j = 1 and the reshape that follows it):
 *                       out[p A + a, s, q C + c] = sum_k x[p, k, q] G[a, k, s, c]
 *                   x [P, K, Q], G [A, K, S, C], out [P A, S, Q C], all contiguous.  The element strides of x (3) and G (4) are
 *                   passed as HOST arrays and checked: anything but the strides of a contiguous tensor (the stride of an
 *                   extent-1 axis is free) is refused with TTR_E_UNSUPPORTED before a byte is read.  The result is written in
 *                   its Kronecker-interleaved layout directly: neither operand is permuted or copied and there is no
 *                   un-permuted intermediate.  A C and P S at most 2^31 - 1.
 * ttr_hsum_step     one mode of the exact K-way chain (metrics.py:407-425):
 *                       W'[a'_1 .. a'_K] = sum_i sum_{a_1 .. a_K} W[a_1 .. a_K] prod_m A_m[a_m, i, a'_m]
 *                   W [r_in[0], .., r_in[K-1]] and W' [r_out[0], .., r_out[K-1]] contiguous, `cores` a HOST array of K device
 *                   pointers A_m [r_in[m], I, r_out[m]], `core_strides` a HOST array of their 3 K element strides, checked as
 *                   above (TTR_E_UNSUPPORTED).  Modes 1 .. K-1 are batched products on strided views -- the mode index i is a
 *                   batch index of the core and a stride-0 index of W: nothing is repeated or permuted -- and the last mode
 *                   contracts (i, a_K) at once, length I r_in[K-1], which sums over i.  1 <= K <= 8.
 *                   Scratch: the intermediates T_m [I, r_out[0 .. m], r_in[m+1 .. K-1]], m = 0 .. K-2, alternate between two
 *                   halves of `workspace`; ttr_hsum_step_workspace_bytes =
 *                       2 * align256( sizeof(dtype) * I * max_m prod_{j <= m} r_out[j] prod_{j > m} r_in[j] )     (0 for K = 1)
 *                   and at most 2^32 bytes: beyond that, or with prod(r_in) / prod(r_out) / I r above 2^31 - 1, the query
 *                   returns TTR_E_UNSUPPORTED (< 0) and so does the entry.  A smaller `workspace_bytes` is TTR_E_WORKSPACE.
 */
int ttr_core_matvec(int dtype, int64_t P, int64_t K, int64_t Q, int64_t A, int64_t S, int64_t C, const void* x,
                    const int64_t* x_strides, const void* G, const int64_t* g_strides, void* out, void* stream);
int64_t ttr_hsum_step_workspace_bytes(int dtype, int64_t K, int64_t I, const int64_t* r_in, const int64_t* r_out);
int ttr_hsum_step(int dtype, int64_t K, int64_t I, const int64_t* r_in, const int64_t* r_out, const void* W,
                  const void* const* cores, const int64_t* core_strides, void* Wout, void* workspace, int64_t workspace_bytes,
                  void* stream);

/*
 * Differential operators on one TT core (ABI 17; derivatives.py:72-130 `partial`, 286-302 `laplacian`): streaming kernels, plain
 * vector loads and stores (16 bytes per lane when C, the strides and the pointers are multiples of 16 bytes, else one element),
 * no host synchronisation, no scratch.  The passes run in fp64 registers for both dtypes, without contraction, and the result is
 * rounded once, at the store: where (inv_step S)^order annihilates the data (S^3 = 0 for I = 3) fp32 input gives exact zeros.
 *
 * S is the reference's I x I central-difference matrix (derivatives.py:96-129): interior rows e[i+1] - e[i-1], row 0 =
 * 2 (e[1] - e[0]) and row I-1 = 2 (e[I-1] - e[I-2]) (its linearly extrapolated edge; I = 1 gives zeros), or, with `periodic`,
 * roll(-1) - roll(+1).  `inv_step` = 1 / step, step = (b1 - b0) / (I + 1) * 2.
 *
 * ttr_mode_diff     Y = (inv_step S)^order X along the middle axis of X [R, I, C] (a Tucker factor [I, R'] is R = 1, C = R').
 *                   X is contiguous: its 3 element strides are passed as a HOST array and checked as ttr_core_matvec checks
 *                   them (TTR_E_UNSUPPORTED before a byte is read; the stride of an extent-1 axis is free).  Y has the element
 *                   strides y_strides = (sr, si, 1) with si >= C and sr >= I si (else TTR_E_UNSUPPORTED): the result can be
 *                   written straight into a block of a wider core, and nothing outside the block is touched.  X == Y,
 *                   order < 1, I < 1 are TTR_E_INVALID.  The lanes walk the flattened (i, c) axis, so the neighbours at +- C are
 *                   contiguous runs for every C.  1 <= order <= ttr_mode_diff_max_order() (= 4) passes run in ONE launch, X
 *                   read from HBM once (2 order + 1 rows per thread in registers); a higher order is TTR_E_UNSUPPORTED: the
 *                   caller chains calls ((inv_step S)^5 = (inv_step S)^1 (inv_step S)^4).
 * ttr_laplace_core  one core of the exact rank-2r train of sum_n (inv_step_n S_n)^2, written whole in one
 *                   launch from one read of X [R, I, C] (contiguous, checked as above), with D = (inv_step S)^2 X:
 *                       pos 0 (first):   out [R, I, 2C]  = [X D]
 *                       pos 1 (middle):  out [2R, I, 2C] = [[X, D], [0, X]]
 *                       pos 2 (last):    out [2R, I, C]  = [D ; X]
 *                   `out` is contiguous; both copies of X are bit-identical to it and the zero block is exactly zero.
 */
int ttr_mode_diff_max_order(void);
int ttr_mode_diff(int dtype, int64_t R, int64_t I, int64_t C, int order, int periodic, double inv_step, const void* X,
                  const int64_t* x_strides, void* Y, const int64_t* y_strides, void* stream);
int ttr_laplace_core(int dtype, int64_t R, int64_t I, int64_t C, int pos, int periodic, double inv_step, const void* X,
                     const int64_t* x_strides, void* out, void* stream);

/*
 * Mode-wise convolution of two TT cores, slice-wise Kronecker in the ranks (added under ABI 17; tools.py:579-647 `convolve`, computed exactly
 * instead of by three cross approximations in the Fourier domain):
 *     out[r1 S1 + s1, k, r2 S2 + s2] = sum_i a[r1, i, r2] c[s1, k + lo - i, s2],   0 <= k < K
 * (terms with k + lo - i outside [0, J) are absent).  `a` [R1, I, R2], `c` [S1, J, S2] and `out` [R1 S1, K, R2 S2] are contiguous;
 * the rank layout is ttr_core_kron's.  (lo, K) is a window of the full result of I + J - 1 entries: 0 <= lo, lo + K <= I + J - 1;
 * only the window is computed.  Before any launch, `out` untouched: TTR_E_INVALID for a bad dtype, a size < 1, a bad window, a
 * null pointer or out == a / out == c; TTR_E_UNSUPPORTED only where an extent, a rank product or the number of workgroups does
 * not fit 32 bits.  No mode size is refused: the sum runs over the shorter mode (min(I, J) terms whichever argument that is),
 * staged in LDS in chunks of at most ttr_core_convolve_max_taps() (= 32) terms, the partial sums staying in registers across the
 * chunks.  A workgroup owns one row (r1, s1), 64 columns and 16 V values of k, V = 4 (fp32) / 2 (fp64) elements of a 16-byte
 * store when R2 S2 is a multiple of V and `out` is 16-byte aligned, else 1.  Accumulation in the input precision (FMA), terms in
 * increasing order of the shorter mode's index; every output is written exactly once, no atomics: bit-identical from run to run.
 * Profiling kind: TTR_PROF_MISC.
 */
int ttr_core_convolve_max_taps(void);
int ttr_core_convolve(int dtype, int64_t R1, int64_t I, int64_t R2, int64_t S1, int64_t J, int64_t S2, int64_t lo, int64_t K,
                      const void* a, const void* c, void* out, void* stream);

/*
 * Enumeration of the strings a mask accepts, level by level (added under ABI 17; automata.py:84-128 `accepted_inputs`, a Python
 * recursion with one matmul per prefix there).  The frontier at mode mu is the productive prefixes in
 * lexicographic order: `L` [P, r] (ALWAYS fp64: path counts are integers and stay exact up to 2^53), `off` [P] the first output
 * row of a prefix and `cnt` [P] its number of output rows (int64).  `dtype` is that of `fiber` / `core`; both are converted to
 * fp64 at the load and accumulated in fp64 (FMA, increasing index).  All arrays are contiguous.
 *
 * ttr_accept_count    C[p, i] = rint(sum_a L[p, a] fiber[a, i])  (int64 [P, I]; saturated at +-2^53), fiber [r, I] the core
 *                     contracted with the right environment of the following modes.
 * ttr_accept_expand   K slots, slot k the child (p, i) = divmod(idx[k], I) (`idx` int64 [K]: the row-major positions of the
 *                     entries C > 0, increasing).  Per slot: Lnew[k, :] = L[p, :] @ core[:, i, :] (fp64 [K, rn]; `Lnew` may be
 *                     null at the last mode: nothing is computed then), offnew[k] = childoff[p, i] (`childoff` int64 [P, I]:
 *                     off[p] + the exclusive scan of C along i), cntnew[k] = C[p, i].  Then every row s < S of Xs (int64
 *                     [S, N]) receives at column mu the symbol of the last slot k with offnew[k] <= s.  Children that are
 *                     not listed are never computed.  `flag` (one int32, zeroed by the caller before the first mode) is ORed
 *                     with TTR_ACCEPT_NEGATIVE where some C[p, i] < 0, TTR_ACCEPT_SUM_MISMATCH where sum_i C[p, i] != cnt[p]
 *                     and TTR_ACCEPT_BAD_INDEX where an idx[k] lies outside [0, P I) (that slot is skipped).  K = 0 checks the
 *                     parents and writes nothing else.
 * Stores are indexed by k < K, s < S and p < P only, whatever the data.  Before any launch: TTR_E_INVALID for a bad dtype, bad
 * sizes, a null pointer, or a rank r / rn above ttr_accept_max_rank() (= 1024: the kernels loop over r per output, untiled);
 * TTR_E_UNSUPPORTED where the frontier does not fit the grid.  No scratch, no host synchronisation.  Profiling kind: TTR_PROF_MISC.
 */
#define TTR_ACCEPT_NEGATIVE 1
#define TTR_ACCEPT_SUM_MISMATCH 2
#define TTR_ACCEPT_BAD_INDEX 4
int ttr_accept_max_rank(void);
int ttr_accept_count(int dtype, int64_t P, int64_t r, int64_t I, const void* L, const void* fiber, void* C, void* stream);
int ttr_accept_expand(int dtype, int64_t P, int64_t r, int64_t I, int64_t rn, int64_t K, int64_t N, int64_t mu, int64_t S,
                      const void* L, const void* core, const void* C, const void* childoff, const void* cnt, const void* idx,
                      void* Lnew, void* offnew, void* cntnew, void* Xs, void* flag, void* stream);

/*
 * Array tools on one TT core (added under ABI 17; ops.py:6-30 `cumsum`, tools.py:266-325 `ttm` with a vector):
 * streaming kernels, no scratch, no host synchronisation, no atomics, 64-bit indices.  A core X [R, I, C] is R slabs of a row-major
 * [I, C] matrix (a Tucker factor [I, S] is R = 1, C = S).  Conventions of ttr_mode_diff: X is contiguous, its 3 element strides
 * are passed as a HOST array and checked (TTR_E_UNSUPPORTED before a byte is read; the stride of an extent-1 axis is free);
 * X == Y, an extent < 1, a bad dtype or a null X / Y / strides are TTR_E_INVALID; Y is untouched by a refused call.
 *
 * ttr_mode_scan    Y[r, i, c] = sum_{i' <= i} X[r, i', c].  Y has the element strides y_strides = (sr, si, 1) with si >= C and
 *                  sr >= I si (else TTR_E_UNSUPPORTED): it can be a block of a wider core, and nothing outside the block is written.
 * ttr_mode_reduce  Y[r, c] = scale * sum_i w[i] X[r, i, c].  `w`: [I] contiguous device elements of the dtype, or NULL (all
 *                  ones).  Y [R, C] has the element strides y_strides = (sr, 1) with sr >= C (else TTR_E_UNSUPPORTED).
 *
 * A thread owns 16 bytes of consecutive c of one row when C is a multiple of that (one 16-byte load / store when the strides
 * and the pointers allow it, else scalar ones with the same arithmetic), else one element.  The lanes of a wave cover up to 64
 * such packs of a row and, where a row has fewer, several consecutive rows (lane = (i_sub, c): contiguous runs down to C = 1),
 * combined by a cross-lane scan / reduction at lane distance C; the carry of a group of rows is the last row of the group before.
 * Where there are fewer than 1024 (r, column tile) items and I is at least 16 row groups, the 16 waves of a workgroup take
 * contiguous chunks of I of one item: the chunk totals pass through LDS and are added in chunk order (the scan reads its chunk
 * twice, the second time from the cache); while such a launch has fewer than 256 workgroups the column tiles are halved, down to
 * one pack, as long as every wave keeps a full row group.  Workgroups never communicate.  Both dtypes accumulate in fp64 registers and round
 * once, at the store; the order of every sum follows from (R, I, C) and the dtype alone: the same call gives the same bits.
 * Profiling kind: TTR_PROF_MISC.
 */
int ttr_mode_scan(int dtype, int64_t R, int64_t I, int64_t C, const void* X, const int64_t* x_strides, void* Y,
                  const int64_t* y_strides, void* stream);
int ttr_mode_reduce(int dtype, int64_t R, int64_t I, int64_t C, const void* X, const int64_t* x_strides, const void* w, double scale,
                    void* Y, const int64_t* y_strides, void* stream);

/*
 * Sparse polynomial-chaos regression (added under ABI 17; interpolation.py:367-383 `PCEInterpolator._design_matrix`, a gather of a
 * P x (C N) intermediate and a product there).  `Z` [P, N]: the centred features, elements of the dtype with
 * the ELEMENT strides (sz0, sz1) -- a column slice of a wider matrix or a transposed view is read where it lies.  `Psi`
 * [N, S, S] contiguous, of the dtype: column s of Psi[n] holds the monomial coefficients of basis polynomial s of mode n.
 * `coords` [C, N] contiguous int64.  The basis value is B(p, n, s) = sum_k Z[p, n]^k Psi[n, k, s], by Horner from k = S - 1 down.
 *
 * ttr_pce_design    M[p ldm + c] = prod_n B(p, n, coords[c, n]), n increasing.  ldm >= C; nothing outside c < C is written.
 * ttr_pce_predict   y[p] = sum_c coef[c] prod_n B(p, n, coords[c, n]), c increasing (one FMA per candidate).  `coef` [C] and
 *                   `y` [P] contiguous, of the dtype.  The P x C matrix is never formed.
 *
 * A workgroup evaluates the N S basis values of a tile of points into LDS once (Psi staged in LDS in chunks of whole modes) and
 * stages the coordinate table in LDS in tiles.  Every coordinate is checked as it is staged: one outside [0, S) makes its
 * candidate's product 0 (whatever the basis values are) and ORs 1 into `flag` (one int32 on the device, zeroed by the caller; a
 * plain store, every writer writes the same bit); no address is formed from an unchecked coordinate.  design: lane =
 * candidate, a point's N S values contiguous in LDS (the gather over s <= 16 consecutive doubles touches distinct banks), the
 * stores of a wave are 64 consecutive c of one row of M.  predict: lane = point, the tile stored [n S + s][point], coordinates and
 * coefficients are wave-uniform reads.  Both dtypes compute in fp64 registers and round once, at the store.  No atomics, no
 * workspace, no host synchronisation, workgroups never communicate; the tiling and with it the order of every product and sum
 * follow from (P, N, S, C) and the dtype alone: the same call gives the same bits.
 * Limits (host-only queries): S <= ttr_pce_max_order() (= 16), N S <= ttr_pce_max_basis() (= 256).  Before any launch, outputs
 * untouched: TTR_E_INVALID for a bad dtype, a size < 1, a size above the limits, ldm < C or a null pointer.
 * Profiling kind: TTR_PROF_MISC.
 */
int ttr_pce_max_order(void);
int ttr_pce_max_basis(void);
int ttr_pce_design(int dtype, int64_t P, int64_t N, int64_t S, int64_t C, const void* Z, int64_t sz0, int64_t sz1, const void* Psi,
                   const void* coords, void* M, int64_t ldm, void* flag, void* stream);
int ttr_pce_predict(int dtype, int64_t P, int64_t N, int64_t S, int64_t C, const void* Z, int64_t sz0, int64_t sz1, const void* Psi,
                    const void* coords, const void* coef, void* y, void* flag, void* stream);

/*
 * The centred, weighted sandwich of the ANOVA / Sobol environment recursion (added under ABI 17; anova.py:99-148 `sobol`, computed
 * from environments instead of masked extended trains), on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64
 * (true fp32 / fp64 operands and accumulators):
 *
 * ttr_mode_sandwich   Q[s, c, c'] = sum_i w[i] sum_{a, b} (A[a, i, c] - mu[a, c]) Z[s, a, b] (A[b, i, c'] - mu[b, c'])
 *
 * `Z` [S, R, R] contiguous (it need not be symmetric), `A` [R, I, C] contiguous -- its 3 element strides are passed as a HOST
 * array and checked (the stride of an extent-1 axis is free) --, `w` [I] contiguous or NULL (all ones), `mu` [R, C] contiguous or
 * NULL (zeros), `Q` [S, C, C] contiguous; all device elements of the dtype.  mu^T Z[s] mu is the same entry with mu as the core
 * [R, 1, C] and `w`, `mu` NULL.  A - mu is formed in the registers that carry the load: no centred copy of the core and no
 * [S, I, R, C] intermediate is written; Y = Z[s] (A_i - mu) stays in accumulator registers and is the operand of the second product.
 * One workgroup owns one s and one contiguous chunk of i (the chunk length follows from (S, I) alone: at least 8, and longer where
 * S ceil(I / 8) exceeds 512 workgroups); with nsplit = ceil(I / chunk) > 1 the chunks' sums go to [S, nsplit, C C] in `workspace`
 * (ttr_mode_sandwich_workspace_bytes, 0 for one chunk; TTR_E_* (< 0) where the entry would refuse the sizes) and ttr_mode_reduce
 * adds them in chunk order.  No atomics, workgroups never communicate, no host synchronisation, 64-bit indices: the same call
 * gives the same bits.
 * Limits: R, C <= ttr_mode_sandwich_max_rank() (= 64; host-only query), S <= 65535; beyond them TTR_E_UNSUPPORTED.  Before any
 * launch, with Q untouched: TTR_E_INVALID for a bad dtype, an extent < 1, a null Z / A / Q / a_strides or a Q that is one of the
 * inputs; TTR_E_UNSUPPORTED for a non-contiguous A; TTR_E_WORKSPACE for a missing or short workspace.
 * Profiling kind: TTR_PROF_MISC.
 */
int ttr_mode_sandwich_max_rank(void);
int64_t ttr_mode_sandwich_workspace_bytes(int dtype, int64_t S, int64_t R, int64_t I, int64_t C);
int ttr_mode_sandwich(int dtype, int64_t S, int64_t R, int64_t I, int64_t C, const void* Z, const void* A, const int64_t* a_strides,
                      const void* w, const void* mu, void* Q, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The minimisation step of TT-cross (added under ABI 17; cross.py:342-359, the `_minimize` branch of `evaluate_function` behind
 * `minimum` / `argmin` / `maximum` / `argmax`): one call per evaluated fibre block, in place, one pass over it.
 *
 * ttr_minimize_step   e[m] <- pi/2 - atan(e[m] - m0) for every m < M = Ra I Rb, and the running best sample updated from e
 *
 * `e` [M] contiguous device elements of the dtype, aligned to the element size (NOT necessarily to 16 bytes: a sliced view is
 * taken where it lies), read as the block [Ra, I, Rb].  The state, on the device: `best` one element of the dtype, `pos` int64 [N]
 * with N = nl + 1 + nr, `flags` int32 [2] = (found, invalid); the caller zeroes `flags` before the first call.  `lset` int64
 * [Ra, nl + 1] with the row stride ld_lset (elements), column 0 unused (cross.py's dummy column); `rset` int64 [Rb, nr + 1] with
 * the row stride ld_rset, last column unused.
 *   m0 = found ? best : 0, read before anything is written; the transform is computed in the dtype (atanf / atan).
 *   m* = the FIRST index at which the original e is smallest among its finite entries (-0.0 and +0.0 compare equal).
 *   A non-finite entry never wins and sets invalid = 1; then `best`, `pos` and `found` are left alone (what such an entry is
 *   transformed to is unspecified; every finite entry is still transformed).  invalid is never cleared.
 *   Otherwise, where !found or e[m*] < best (strictly): best = e[m*] (the sample itself), found = 1, and with
 *   m* = (a I + i) Rb + c: pos = lset[a, 1:] ++ [i] ++ rset[c, :-1].  Else `best`, `pos` and `found` are not written.
 * Two launches on `stream`: a streaming pass (16-byte loads and stores on the aligned part of e; a workgroup owns whole chunks of
 * TTR_MINIMIZE_BLOCK_ELEMS consecutive elements, chunk c going to workgroup c mod 2048; per lane the lexicographic minimum of
 * (value, index), combined across the wave and through LDS; one partial per workgroup into `workspace`), then one workgroup that
 * reduces the partials and updates the state.  All comparisons are exact and (value, index) is a total order: the result does not
 * depend on the reduction order, the same call gives the same bits.  No atomics, no host synchronisation, 64-bit indices.
 * ttr_minimize_workspace_bytes(dtype, M): the bytes of `workspace` (8-byte aligned); TTR_E_INVALID (< 0) for a bad dtype or M < 1.
 * Before any launch, with e and the state untouched: TTR_E_INVALID for a bad dtype, an extent < 1, nl or nr < 0, a row stride
 * below its row length, a null or misaligned pointer; TTR_E_UNSUPPORTED for a block or index set beyond 2^57 elements;
 * TTR_E_WORKSPACE for a missing or short workspace.  Profiling kind: TTR_PROF_MISC.
 */
#define TTR_MINIMIZE_BLOCK_ELEMS 4096
int64_t ttr_minimize_workspace_bytes(int dtype, int64_t M);
int ttr_minimize_step(int dtype, void* e, int64_t Ra, int64_t I, int64_t Rb, const void* lset, int64_t ld_lset, int64_t nl,
                      const void* rset, int64_t ld_rset, int64_t nr, void* best, void* pos, void* flags, void* workspace,
                      int64_t workspace_bytes, void* stream);

/*
 * One mode of sampling from a train read as an unnormalised mass function (added under ABI 17; tools.py:362-407 `sample`, which
 * forms the P x I matrix lefts @ fiber and passes over it about ten times): one launch per mode, the matrix
 * never exists in global memory and there is no workspace.
 *
 * ttr_sample_step     per sample p < P, with q[i] = |sum_a L[p, a] fiber[a, i]| computed in the dtype on the matrix cores and the
 *                     running sum c_i = q[0] + .. + q[i] and T = c_{I-1} in fp64 whatever the dtype:
 *                       X[p stride_x] = the smallest i with c_i > u[p stride_u] T (compared in fp64); where the rounding of u T
 *                                       leaves none, the last i with q[i] > 0
 *                       Lnew[p, :]    = (L[p, :] @ core[:, x, :]) / T, the product an fma chain in the dtype, the quotient in
 *                                       fp64, rounded once at the store; not computed when Lnew is NULL (the last mode)
 *
 * `L` [P, r] with the row stride ldl (elements; unit column stride), `fiber` [r, I] contiguous (the core times the right vector
 * of the next mode: an input, as in ttr_accept_count), `core` [r, I, rn] with the element strides core_strides[3] (a HOST array;
 * the last must be 1, the others >= 0, the stride of an extent-1 axis is free), `u` fp64 thresholds in [0, 1), `X` int64,
 * `Lnew` [P, rn] with the row stride ldn.  `flag` is one int32 device word, zeroed by the caller before the first mode and ORed
 * only where a check of a sample fails: TTR_SAMPLE_ZERO_TOTAL (T == 0), TTR_SAMPLE_NONFINITE (T not finite),
 * TTR_SAMPLE_BAD_THRESHOLD (u outside [0, 1) or NaN).  A flagged sample stores X = -1 and a zero row of Lnew.
 * A workgroup owns TTR_SAMPLE_TILE_F32 / _F64 samples (a wave a quarter of them) and forms q in blocks of TTR_SAMPLE_BLOCK_F32 /
 * _F64 columns of fiber; the running sum is sequential over the columns in segments of 16 (fp32) / 4 (fp64): inside a segment
 * from the segment's own partial sums, from segment to segment by their totals.  Every store is indexed by the sample's own p;
 * the only data-dependent address is the LOAD of core[:, x, :] with 0 <= x < I.  X[p] and Lnew[p, :] depend on the inputs of
 * sample p alone: not on P, on the other samples or on its place in a tile; the same call gives the same bits.
 * ttr_sample_max_rank(): the largest r and rn.
 * Before any device call: TTR_E_INVALID for a bad dtype, P < 0, an extent < 1, a rank above the limit, a null pointer (Lnew
 * excepted); TTR_E_UNSUPPORTED for a core whose last stride is not 1 or with a negative stride, ldl < r, ldn < rn, stride_u or
 * stride_x < 1, I or P beyond 2^31 - 64 columns / 2^35 samples.  P == 0 returns at once.  Profiling kind: TTR_PROF_MISC.
 */
#define TTR_SAMPLE_ZERO_TOTAL 1
#define TTR_SAMPLE_NONFINITE 2
#define TTR_SAMPLE_BAD_THRESHOLD 4
#define TTR_SAMPLE_TILE_F32 128
#define TTR_SAMPLE_TILE_F64 64
#define TTR_SAMPLE_BLOCK_F32 32
#define TTR_SAMPLE_BLOCK_F64 16
int ttr_sample_max_rank(void);
int ttr_sample_step(int dtype, int64_t P, int64_t r, int64_t I, int64_t rn, const void* L, int64_t ldl, const void* fiber,
                    const void* core, const int64_t* core_strides, const void* u, int64_t stride_u, void* X, int64_t stride_x,
                    void* Lnew, int64_t ldn, void* flag, void* stream);

/*
 * One step of the product of a TT-matrix or a CP-matrix with a dense batch (added under ABI 17; matrix.py:420-443 `tt_multiply` and
 * 446-468 `cp_multiply`, chains of d einsum calls, each a permuted copy of the running intermediate and a GEMM).
 * With the reference's index order the row-major output of step k IS the input of step k + 1: Y [D, O, S] read as
 * [I', D', S] with D = I' D'' and D' = (D'', O).  Nothing is permuted, padded or copied, and there is no workspace.
 *
 * ttr_ttm_step   Y[dd, o, s] = sum_i sum_r X[i, dd, r] G[r, i, o, s].  `X` [I, D, R], `G` [R, I, O, S] (a TTMatrix core) and `Y`
 *                [D, O, S] are contiguous; the element strides of X (3) and of G (4) are passed as HOST arrays and checked as
 *                ttr_core_matvec checks them: TTR_E_UNSUPPORTED before a byte is read, the stride of an extent-1 axis is free.
 *                A GEMM with M = D, N = O S and K = I R on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 (operands and
 *                accumulators in the dtype) whose K index k = i R + r has two strides in X: X is read in place, in runs of equal i,
 *                so a quad of k that straddles two i (every R that is no multiple of 4) takes its halves from their own
 *                addresses.  A workgroup owns TTR_TTM_TILE_M x TTR_TTM_TILE_N of Y and walks K in tiles of TTR_TTM_TILE_K
 *                through LDS; column tiles of 16 past N and quads of k past K are not multiplied (N < 16: the last step; K < 4:
 *                the first step of a small mode).  Any I, D, R, O, S >= 1 with D, I R and O S at most 2^31 - 1 (beyond that
 *                TTR_E_UNSUPPORTED): no rank limit, 64-bit element offsets.  No atomics, no split of K across workgroups: every
 *                element of Y is one accumulation chain in increasing k, its order fixed by the five extents and the dtype; the
 *                same call gives the same bits.  Profiling kind: TTR_PROF_GEMM.
 * ttr_cpm_step   Y[dd, o, r] = sum_i X[i, dd, r] C[i, o, r] (x_has_rank = 1) or sum_i X[i, dd] C[i, o, r] (x_has_rank = 0: the
 *                first step, X broadcast over r).  `X` [I, D, R] or [I, D], `C` [I, O, R] (a CPMatrix core), `Y` [D, O, R]: all
 *                contiguous.  A streaming kernel on the vector ALUs: 16-byte accesses along r where R is a multiple of 16 bytes of
 *                elements and the pointers are 16-byte aligned, else scalar ones with the same arithmetic (the bits do not depend
 *                on where the buffers lie); the sum over i is an fma chain from 0 in increasing i.  The final sum over r of
 *                `cp_multiply` is ttr_mode_reduce (R = D O, I = rank, C = 1).  Profiling kind: TTR_PROF_MISC.
 * Before any launch, with Y untouched: TTR_E_INVALID for a bad dtype, an extent < 1, an x_has_rank other than 0 / 1, a null
 * pointer or a Y that is one of the inputs; TTR_E_UNSUPPORTED for strides other than the contiguous ones and for an operand of
 * 2^57 elements or more.
 */
#define TTR_TTM_TILE_M 64
#define TTR_TTM_TILE_N 64
#define TTR_TTM_TILE_K 32
int ttr_ttm_step(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S, const void* X, const int64_t* x_strides,
                 const void* G, const int64_t* g_strides, void* Y, void* stream);
int ttr_cpm_step(int dtype, int64_t I, int64_t D, int64_t O, int64_t R, int x_has_rank, const void* X, const void* C, void* Y,
                 void* stream);

/*
 * The backward of ttr_ttm_step (added under ABI 17; what torch autograd derives from the einsum chain of matrix.py:420-443
 * `tt_multiply`).  X [I, D, R], G [R, I, O, S], dY [D, O, S], dX [I, D, R] and dG [R, I, O, S] are all
 * contiguous (there are no stride arguments).  dX of step k, as it lies, is dY of step k - 1: the backward chain copies nothing.
 *
 * ttr_ttm_grad_input   dX[i, dd, r] = sum_{o, s} dY[dd, o, s] G[r, i, o, s].  A GEMM with M = D, N = I R and K = O S, K contiguous
 *                      in both operands and never split across workgroups; the 64 x 64 output tile is staged in LDS and stored
 *                      in runs of equal i (the mirror of ttr_ttm_step's two-stride load), in 16-byte packs where R is a multiple
 *                      of 16 bytes of elements and dX is 16-byte aligned.
 * ttr_ttm_grad_core    dG[r, i, o, s] = sum_dd X[i, dd, r] dY[dd, o, s].  M = I R (two-stride load), N = O S, K = D, cut into
 *                      slabs of ttr_ttm_grad_core_slab_rows rows; a workgroup owns one (64 x 64 tile, slab) pair.  The slab rule
 *                      reads the six arguments only, never the device: with tiles = ceil(I R / 64) ceil(O S / 64) and
 *                      want = max(1, 1024 / tiles), slab_rows = max(256, ceil(D / want) rounded up to a multiple of 32).  One
 *                      slab (D <= slab_rows): dG is written directly, `workspace` may be null.  Several: the partial tiles go to
 *                      `workspace` [nslab, I R, O S] (ttr_ttm_grad_core_workspace_bytes; 0 for one slab) and a second launch sums
 *                      them in slab order: eight runs of ceil(nslab / 8) consecutive slabs, each summed in increasing slab
 *                      order, the run sums then added in run order (an association fixed by nslab alone).  A missing or short
 *                      workspace is TTR_E_WORKSPACE.
 * Both run on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 with operands and accumulators in the dtype and 64-bit element
 * offsets; column tiles of 16 past N and quads of k past K are not multiplied.  No atomics, no host synchronisation: the same
 * call gives the same bits, wherever the buffers lie.  Before any launch, with the output untouched: TTR_E_INVALID for a bad
 * dtype, an extent below 1, a null pointer or an output that is one of the inputs; TTR_E_UNSUPPORTED for D, I R or O S above
 * 2^31 - 1 and for an operand of 2^57 elements or more (the two queries return the same codes, < 0).  Profiling kind:
 * TTR_PROF_GEMM.
 */
int ttr_ttm_grad_input(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S, const void* dY, const void* G, void* dX,
                       void* stream);
int64_t ttr_ttm_grad_core_slab_rows(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S);
int64_t ttr_ttm_grad_core_workspace_bytes(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S);
int ttr_ttm_grad_core(int dtype, int64_t I, int64_t D, int64_t R, int64_t O, int64_t S, const void* X, const void* dY, void* dG,
                      void* workspace, int64_t workspace_bytes, void* stream);

/*
 * One step of the row lookup of a TT-matrix, M[rows, :] without the dense matrix (added under ABI 17; lookup.py `tt_lookup`;
 * DESIGN section 27):
 *
 *   Y[p, dd, o, s] = sum_r X[xrow ? xrow[p] : p, dd, r] * G[r, idx[p], o, s]
 *
 * `X` [rows_x, D, R] and `Y` [P, D, O, S] are contiguous; Y of a step, read as [P, D O, S], is the X of the next one as it lies.
 * `G` [R, I, O, S] (a TTMatrix core) has the four element strides g_strides, a HOST array: a unit stride along S and no negative
 * stride are needed (else TTR_E_UNSUPPORTED before a byte is read; the stride of an extent-1 axis is free), so a sliced or
 * permuted view of a core is read where it lies.  `idx` and `xrow` are int64 device vectors of P entries, BOTH with the element
 * stride `stride_idx`: two columns of one [P, d] digit table (stride d), or two contiguous vectors (stride 1).  `xrow` may be
 * NULL: sample p then reads X[p].  idx wraps negative values as in torch (-I <= idx < I); xrow does not (0 <= xrow < rows_x).
 *
 * The indices are validated on the device first: a bad entry ORs the int32 device word *oob_flag with 1, and then nothing else is
 * written.  The word is NOT cleared by the call -- the steps of a chain share one word, cleared by the caller before the first
 * and read after the last -- and when it is set on entry the call writes nothing.  No host synchronisation.
 *
 * The samples are grouped by idx on the device (a counting sort: histogram, scan, scatter of the sample ids into `workspace`;
 * ttr_ttm_lookup_workspace_bytes(P, I) bytes, < 0 for P < 0 or an I outside 1 .. 2^31 - 1), so that the samples of a group share
 * their R x (O S) slice: a workgroup owns 64 (sample, dd) rows x 64 columns of one group, stages the gathered X rows and the
 * slice through LDS in chunks of 32 r and multiplies on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 (operands and
 * accumulators in the dtype).  Rows past the group, column tiles of 16 past O S and quads of r past R are zero-filled in LDS or
 * skipped, never read out of bounds.  Every element of Y is one accumulation chain in increasing r whose order depends on R and
 * the dtype alone: a row's bits do not depend on P, on the other samples, on the order inside a group or on xrow being NULL or
 * the identity.  No atomics on floating-point data.  No rank limit, 64-bit element offsets.  Profiling kind: TTR_PROF_GEMM.
 *
 * Before any launch, with Y untouched: TTR_E_INVALID for a bad dtype, an extent < 1 (P = 0 returns TTR_OK at once), a
 * stride_idx < 1, a null pointer (xrow excepted) or a Y that is one of the inputs; TTR_E_UNSUPPORTED for the strides of G above,
 * for D R, O S, P D, I or rows_x above 2^31 - 1 and for an operand of 2^57 elements or more; TTR_E_WORKSPACE for a missing or
 * short workspace.
 */
int64_t ttr_ttm_lookup_workspace_bytes(int64_t P, int64_t I);
int ttr_ttm_lookup_step(int dtype, int64_t P, int64_t rows_x, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S,
                        const void* X, const void* xrow, const void* G, const int64_t* g_strides, const void* idx,
                        int64_t stride_idx, void* Y, void* oob_flag, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The backward of ttr_ttm_lookup_step and the segmented row sum of the trainable TT embedding (added under ABI 17; embedding.py
 * `tt_embedding`, `tt_embedding_bag`).  With X [rows_x, D, R], dY [P, D, O, S] and dX [P, D, R] contiguous, dG
 * [R, I, O, S] contiguous, and `idx`, `xrow`, `stride_idx` and `oob_flag` as in ttr_ttm_lookup_step:
 *
 *   ttr_ttm_lookup_grad_core    dG[r, i, o, s] = sum_{p: idx[p] = i} sum_dd X[xrow ? xrow[p] : p, dd, r] * dY[p, dd, o, s]
 *   ttr_ttm_lookup_grad_input   dX[p, dd, r]   = sum_{o, s} dY[p, dd, o, s] * G[r, idx[p], o, s]
 *
 * `perm` is a contiguous int64 device vector of P entries: the sample ids 0 .. P - 1 grouped by wrapped idx (group 0 first; the
 * order inside a group is the caller's, a stable sort keeps the sample order).  Neither entry sorts: each counts the groups
 * (histogram and scan on the device, into `workspace`; no readback) and reads its rows through perm.  idx (wrapped), perm and
 * xrow (not wrapped) are validated on the device first: a bad entry ORs *oob_flag with 1 and then nothing else is written, as when
 * the word is set on entry; the word is never cleared.  No host synchronisation, no atomics on floating-point data, no rank
 * limit, 64-bit element offsets; v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 with operands and accumulators in the dtype.
 *
 * ttr_ttm_lookup_grad_core: slice i is one GEMM with M = R, N = O S and K = cnt_i D, the K rows gathered D R resp. D N contiguous
 * elements per sample; a workgroup owns a 64 x 64 tile of (r, n) and one SLAB of the slice's K range, walked in chunks of 32.  The
 * slab length ttr_ttm_lookup_grad_core_slab_rows(dtype, P, D, R, I, O, S) reads its arguments only: with tiles = ceil(R / 64)
 * ceil(O S / 64) and want = max(1, 1024 / tiles), slab_rows = max(256, ceil(P D / want) rounded up to a multiple of 32).  Slice i
 * has ceil(cnt_i D / slab_rows) slabs, numbered by a scan on the device.  A slice of one slab writes dG directly; the slabs of the
 * others write partial tiles to the workspace, and a second launch adds a slice's partials in increasing slab order (one chain
 * per element) and writes exact zeros for a slice without samples.  The workspace (ttr_ttm_lookup_grad_core_workspace_bytes)
 * holds the counts and ceil(P D / slab_rows) + I partial tiles of R x O S, the host-side upper bound of the slab count.  The same
 * inputs and the same perm give the same bits, and so do xrow = NULL and the identity map, wherever the buffers lie.  P = 0
 * zeroes dG.
 *
 * ttr_ttm_lookup_grad_input: ttr_ttm_lookup_step's structure with the slice staged transposed: the rows of a group are the
 * (sample, dd) pairs of its samples in tiles of 64, K = (o, s) is the contiguous axis of dY and of G and N = R.  `G` is read with
 * the four element strides g_strides under ttr_ttm_lookup_step's rules.  K is never split: every element of dX is one chain in
 * increasing (o, s) fixed by O S and the dtype, so a row's bits do not depend on P, on the other samples or on the order inside
 * a group.  Workspace: ttr_ttm_lookup_grad_input_workspace_bytes(P, I) (< 0 for P < 0 or an I outside 1 .. 2^31 - 1).  P = 0
 * returns TTR_OK at once.
 *
 * Before any launch, with the output untouched: TTR_E_INVALID for a bad dtype, an extent < 1 (P < 0), a stride_idx < 1, a null
 * pointer (xrow excepted) or an output that is one of the inputs; TTR_E_UNSUPPORTED for the strides of G, for D R, O S, P D, I or
 * rows_x above 2^31 - 1 and for an operand of 2^57 elements or more (the queries return the same codes, < 0); TTR_E_WORKSPACE
 * for a missing or short workspace.  Profiling kind: TTR_PROF_GEMM.
 *
 * ttr_segment_sum   out[b, :] = sum_{q = seg[b]}^{seg[b + 1] - 1} (w ? w[src(q)] : 1) * Y[src(q), :],   src(q) = perm ? perm[q] : q
 *
 * `Y` [P, C] and `out` [B, C] are contiguous, `w` [P] (or NULL: ones) has the dtype, `perm` [P] (or NULL) and `seg` [B + 1] are
 * contiguous int64 device vectors, seg non-decreasing in 0 .. P.  A workgroup owns one segment and one block of columns (16-byte
 * loads where C is a multiple of 16 bytes of elements and Y and out are 16-byte aligned); its four waves take consecutive quarters
 * of the segment and are combined in wave order.  Accumulation is in fp64 with one rounding at the store (fp32: exact products;
 * fp64: compensated sums), in a fixed order: the same call gives the same bits.  An empty segment gives zeros.  A segment is never
 * split across workgroups: a very long one sits on ceil(C / block) of them.  seg is clamped to 0 .. P and a src outside 0 .. P - 1
 * is skipped, never read.  Before any launch: TTR_E_INVALID for a bad dtype, B < 0, P < 0, C < 1, a null pointer (w and perm
 * excepted; Y where P = 0) or an out that is one of the inputs; TTR_E_UNSUPPORTED for an operand of 2^57 elements or more.  B = 0
 * returns TTR_OK at once.  Profiling kind: TTR_PROF_MISC.
 */
int64_t ttr_ttm_lookup_grad_core_slab_rows(int dtype, int64_t P, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S);
int64_t ttr_ttm_lookup_grad_core_workspace_bytes(int dtype, int64_t P, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S);
int ttr_ttm_lookup_grad_core(int dtype, int64_t P, int64_t rows_x, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S,
                             const void* X, const void* xrow, const void* dY, const void* idx, int64_t stride_idx,
                             const void* perm, void* dG, void* oob_flag, void* workspace, int64_t workspace_bytes, void* stream);
int64_t ttr_ttm_lookup_grad_input_workspace_bytes(int64_t P, int64_t I);
int ttr_ttm_lookup_grad_input(int dtype, int64_t P, int64_t D, int64_t R, int64_t I, int64_t O, int64_t S, const void* dY,
                              const void* G, const int64_t* g_strides, const void* idx, int64_t stride_idx, const void* perm,
                              void* dX, void* oob_flag, void* workspace, int64_t workspace_bytes, void* stream);
int ttr_segment_sum(int dtype, int64_t B, int64_t P, int64_t C, const void* Y, const void* w, const void* perm, const void* seg,
                    void* out, void* stream);

/*
 * One core of a TT-matrix product that stays in TT format (added under ABI 17; ttalgebra.py `tt_apply`, `tt_matmul`; DESIGN
 * section 28):
 *     out[r S1 + a, p, q, s S2 + b] = sum_j A[r, p, j, s] B[a, j, q, b]
 * `A` [R1, P, J, R2], `B` [S1, J, Q, S2] and `out` [R1 S1, P, Q, R2 S2] are contiguous; the rank layout is ttr_core_kron's (the
 * first operand's rank major).  P = 1 is a core of vec(t) @ M (A the train's core, B the matrix core), Q = 1 one of M @ vec(u),
 * the general case one of the product of two TT-matrices.  A GEMM with M = (r, p, s), N = (a, q, b) and K = J whose output, E =
 * R1 S1 P Q R2 S2 elements, is written once for 2 J E flops while the small operands are re-read from the cache: a store kernel
 * for the J of a mode.  A workgroup owns TTR_COMPOSE_TILE_M rows x TTR_COMPOSE_TILE_N columns (s resp. b fastest) and walks J in
 * chunks of TTR_COMPOSE_TILE_K through LDS, on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 (operands and accumulators in
 * the dtype; quads of j, the tail zero-filled).  The accumulators are staged through LDS and written in memory order --
 * (segment of equal (a, q), row, b): consecutive lanes are consecutive addresses along the runs of R2 S2 elements a fixed
 * (r, a, p, q) has -- in 16-byte packs where S2 is a multiple of 16 bytes of elements (every row of a run then starts on a
 * pack) and `out` is 16-byte aligned, else in scalar stores with the same arithmetic and order.  Every element is one
 * accumulation chain from 0 in increasing j: its bits do not depend on its place in a tile, on the other extents or on the
 * alignment of `out`.  Every element is written exactly once; no atomics, no workspace, no rank limit, 64-bit element offsets.
 * Before any launch, `out` untouched: TTR_E_INVALID for a bad dtype, an extent < 1, a null pointer or out == A / out == B;
 * TTR_E_UNSUPPORTED only where an extent, a rank product (R1 S1, R2 S2) or the number of workgroups does not fit 32 bits, or
 * an operand has 2^57 elements or more.  Profiling kind: TTR_PROF_GEMM.
 */
#define TTR_COMPOSE_TILE_M 64
#define TTR_COMPOSE_TILE_N 64
#define TTR_COMPOSE_TILE_K 32
int ttr_core_compose(int dtype, int64_t R1, int64_t P, int64_t J, int64_t R2, int64_t S1, int64_t Q, int64_t S2, const void* A,
                     const void* B, void* out, void* stream);

/*
 * Half of a three-layer environment application, the hot path of the ALS solver (added under ABI 17; ttsolve.py `tt_solve`;
 * DESIGN section 29):
 *     H[r, i, a', s'] = sum_{a, j} G[a, i, j, a'] * ( sum_{r'} Phi[r, a, r'] * X[r', j, s'] )
 * `Phi` [R, A, R'] (an interface of bra, matrix and ket) and `H` [R, I, A', S'] are contiguous.  `X` [R', J, S'] (a ket core) has
 * the three element strides x_strides and `G` [A, I, J, A'] (a TT-matrix core) the four element strides g_strides, both HOST
 * arrays: any non-negative strides are read where they lie (a tt_transpose view, the rank-swapped views of a right-to-left
 * sweep); a negative stride, or strides that span 2^57 elements or more, are TTR_E_UNSUPPORTED before a byte is read, and the
 * stride of an extent-1 axis is free.
 * With H laid out this way both of its consumers are plain ttr_gemm calls on H as it lies: the local matvec
 * y[r, i, s] = sum_{a', s'} H[r, i, a', s'] Psi[s, a', s'] (M = R I, K = A' S', N = S, second operand transposed) and the
 * environment update Phi'[s, a', s'] = sum_{r, i} Y[r, i, s] H[r, i, a', s'] (first operand transposed).
 * The intermediate T[r, (a, j), s'] never reaches global memory: a workgroup owns TTR_ENV_TILE_R r x TTR_ENV_TILE_S s' x
 * TTR_ENV_TILE_N columns (i, a') of H, walks k = a J + j in chunks of TTR_ENV_TILE_K, computes the chunk's T tiles (sums over r',
 * operands straight from memory) into LDS and multiplies them with the staged chunk of G; both contractions run on
 * v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 with operands and accumulators in the dtype.  Stage 1 is recomputed once per
 * column tile.  Everything past an extent is a zero in LDS or is skipped, never read.  No workspace, no atomics, no split of
 * either sum across workgroups, no rank limit, 64-bit element offsets.  Every element of H is one chain -- the inner sums from 0
 * in increasing r', the outer from 0 in increasing (a, j) -- fixed by R', A, J and the dtype: the same call gives the same bits,
 * and an element's bits do not depend on its place in a tile or on R, S', I, A'.
 * Before any launch, with H untouched: TTR_E_INVALID for a bad dtype, an extent < 1, a null pointer or an H that is one of the
 * inputs; TTR_E_UNSUPPORTED for the strides above, for an extent, A J, I A' or a number of workgroups beyond 2^31 - 1 and for an
 * operand of 2^57 elements or more.  Profiling kind: TTR_PROF_GEMM.
 */
#define TTR_ENV_TILE_R 16
#define TTR_ENV_TILE_S 16
#define TTR_ENV_TILE_N 64
#define TTR_ENV_TILE_K 16
int ttr_env_half_apply(int dtype, int64_t R, int64_t A, int64_t Rp, int64_t J, int64_t Sp, int64_t I, int64_t Ap, const void* Phi,
                       const void* X, const int64_t* x_strides, const void* G, const int64_t* g_strides, void* H, void* stream);

/*
 * One Rayleigh-Ritz step of a three-vector LOBPCG in two launches, the local eigensolver of the ALS eigenvalue solver (added under
 * ABI 17; tteigs.py `tt_eigsh`).  The state of a local problem B v = theta v is six contiguous vectors of n
 * elements in the dtype: X, AX = B X, W (the residual AX - theta X), AW = B W (the caller's matvec), P and AP (the previous
 * direction).  None of the six may overlap another.
 *
 * ttr_ritz_parts / ttr_ritz_workspace_bytes: the number of workgroups of the Gram launch, 1 + (ceil(n / V) - 1) / 1024 capped at
 * TTR_RITZ_MAX_PARTS with V = 16 bytes / element size, and the bytes of `part`, 12 doubles per workgroup.  Both are functions of
 * n and the dtype alone, so the association of every sum is fixed by n and the dtype.  TTR_E_INVALID (negative) for a bad dtype
 * or n < 1.
 *
 * ttr_ritz_gram: part[g][0..12) = workgroup g's share of S = V^T V and T = V^T A V for V = [X W P], upper triangles:
 *     S_xx S_xw S_xp S_ww S_wp S_pp   T_xx = X.AX  T_xw = X.AW  T_xp = X.AP  T_ww = W.AW  T_wp = W.AP  T_pp = P.AP
 * One pass over the vectors; products and sums in double (one fma per product); 16-byte packs where every pointer is 16-byte
 * aligned, element loads with the same arithmetic otherwise and for the last pack of an n that is no multiple of V.  Pack p belongs
 * to thread p % 256 of workgroup (p / 256) % parts, which adds its packs in increasing p; lanes meet in the library's wave sum, the
 * four waves in increasing order.  The same call gives the same bits, aligned or not.  No atomics.
 * mode TTR_RITZ_INIT reads only X and AX and fills S_xx and T_xx (the other ten are zeros; W .. AP may be NULL); in
 * TTR_RITZ_STEP P and AP may both be NULL: zeros, not read.
 *
 * ttr_ritz_update: every workgroup adds the rows of `part` in increasing g (the previous launch's reduction, finished in this
 * one's prologue), one thread solves the pencil in double, and the workgroup updates its slice of the vectors in place, every
 * element read and written by the same thread.
 *   TTR_RITZ_INIT   X <- X / ||X||, AX <- AX / ||X||, theta' = T_xx / S_xx, W <- AX - theta' X, P <- AP <- 0 (AW is not read;
 *                   P and AP may both be NULL)
 *   TTR_RITZ_STEP   res = sqrt(S_ww / (S_ww + theta^2 S_xx)) with theta = T_xx / S_xx, the incoming ||W|| / ||AX|| (0 for
 *                   S_ww = 0).  res <= rel: the step is FROZEN and writes no vector.  Otherwise the extreme Ritz pair (`which`:
 *                   TTR_RITZ_SA the smallest, TTR_RITZ_LA the largest) of (T, S): S is scaled to unit diagonal, a zero diagonal
 *                   dropping its direction; the eigendirections of the scaled S below TTR_RITZ_DROP eps (eps of the dtype) of
 *                   its largest eigenvalue are dropped; the whitened problem is solved (cyclic Jacobi); the coefficients c are
 *                   scaled to c^T S c = 1 with c0 >= 0 and theta' = c^T T c.  Then
 *                       Pn = c1 W + c2 P, APn = c1 AW + c2 AP, X <- c0 X + Pn, AX <- c0 AX + APn, P <- Pn, AP <- APn,
 *                       W <- AX - theta' X   (of the rounded new X and AX)
 *                   evaluated in double and rounded once.  P and AP both NULL: zeros, neither read nor written.
 * Workgroup 0 overwrites state[0..8) = theta', res, frozen, flags (1: a non-finite sum, 2: S_xx == 0; a flagged step writes no
 * vector and has theta' = 0), c0, c1, c2, the number of directions kept (0 for a frozen or flagged step, whose c is (1, 0, 0)),
 * and accumulates sweep[0..4): [0] = max([0], res) when `first` is set, [1] += (flags != 0), [2] = theta', [3] |= flags (as an
 * integer).  Nothing is read back.
 *
 * Before any launch: TTR_E_INVALID for a bad dtype, mode or `which`, n < 1, rel < 0, a null pointer (or only one of P and AP);
 * TTR_E_WORKSPACE for workspace_bytes below ttr_ritz_workspace_bytes; TTR_E_UNSUPPORTED for n of 2^57 or more.
 * `part` given to ttr_ritz_update must hold the ttr_ritz_parts(dtype, n) rows ttr_ritz_gram wrote for the same n and dtype.
 * Profiling kind: TTR_PROF_MISC.
 */
#define TTR_RITZ_INIT 0
#define TTR_RITZ_STEP 1
#define TTR_RITZ_SA 0
#define TTR_RITZ_LA 1
#define TTR_RITZ_MAX_PARTS 256
#define TTR_RITZ_DROP 64
int ttr_ritz_parts(int dtype, int64_t n);
int64_t ttr_ritz_workspace_bytes(int dtype, int64_t n);
int ttr_ritz_gram(int dtype, int mode, int64_t n, const void* X, const void* AX, const void* W, const void* AW, const void* P,
                  const void* AP, double* part, int64_t workspace_bytes, void* stream);
int ttr_ritz_update(int dtype, int mode, int which, int first, int64_t n, double rel, const double* part, void* X, void* AX, void* W,
                    const void* AW, void* P, void* AP, double* state, double* sweep, void* stream);

/*
 * One conjugate-gradient step in three launches, the local solver of the rank-adaptive AMEn solver (added under ABI 17;
 * ttamen.py `tt_amen_solve`; ttsolve.py `_cg` is the specification of the recurrences).  The state of a local
 * system B x = f is four contiguous vectors of n elements in the dtype: the iterate v, the residual r, the direction p and
 * Bp = B p (the caller's matvec, between ttr_cg_direction of one step and ttr_cg_dot of the next).  None of the vectors of one
 * call may overlap another.  Step s (`step`, counted from 0; only its parity is used) is
 *     pBp = p . Bp;  active = rs > thr2;  good = pBp > 0;  live = active & good;  alpha = live ? rs / pBp : 0
 *     v += alpha p;  r -= alpha Bp;  rs' = r . r;  beta = live ? rs' / max(rs, tiny) : 0;  p = r + beta p;  rs <- rs'
 * with tiny the smallest normal number of the dtype.  A step that is not live (frozen: rs <= thr2, or pBp <= 0) writes NO vector
 * and carries rs over.
 *
 * state, fp64[8], the caller's, set before step 0 to (rs, anything, thr2, 0, ...):
 *     [0], [1]   rs: step s reads slot s & 1, its ttr_cg_direction writes slot 1 - (s & 1), which step s + 1 reads
 *     [2]        thr2 = rel^2 f . f: read, never written
 *     [3]        += 1 per step with rs > thr2 and pBp <= 0 (a lost positive definiteness): read and written by one thread
 *     [4] .. [6] live (1 or 0), alpha and pBp of the last ttr_cg_update
 *     [7]        beta of the last ttr_cg_direction
 * No launch reads a word that another workgroup of the same launch writes: ttr_cg_update reads [s & 1] and [2] and writes
 * [3] .. [6]; ttr_cg_direction reads [s & 1] and [4] and writes [1 - (s & 1)] and [7].  All scalars stay on the device.
 *
 * ttr_cg_parts / ttr_cg_workspace_bytes: the number of workgroups of each of the three launches, the rule of ttr_ritz_parts
 * (1 + (ceil(n / V) - 1) / 1024 capped at TTR_CG_MAX_PARTS, V = 16 bytes / element size), and the bytes of `part`, two rows of
 * `parts` doubles (row 0: the shares of p . Bp, row 1: of r . r).  Both are functions of n and the dtype alone.  TTR_E_INVALID
 * (negative) for a bad dtype or n < 1.
 *
 * ttr_cg_dot: part[0][g] = workgroup g's share of p . Bp.  Products and sums in double, one fma per product; 16-byte packs where
 * both pointers are 16-byte aligned, element loads with the same arithmetic otherwise and for the last pack of an n that is no
 * multiple of V.  Pack q belongs to thread q % 256 of workgroup (q / 256) % parts, which adds its packs in increasing q; lanes
 * meet in the library's wave sum, the four waves in increasing order.
 * ttr_cg_update: every workgroup adds part[0][*] in increasing g (the previous launch's reduction, finished in this one's
 * prologue), forms alpha in double, and updates its slice of v and r in place: evaluated in double (one fma), rounded once, every
 * element read and written by the same thread.  It writes its share of r . r, of the ROUNDED r, to part[1][g] (a step that is
 * not live: zeros).  The first thread of workgroup 0 writes state[3] .. [6].
 * ttr_cg_direction: every workgroup adds part[1][*] in increasing g, forms beta, and writes its slice of p = r + beta p; the first
 * thread of workgroup 0 stores the next rs (rs' of a live step, rs otherwise) and beta.
 * The same call gives the same bits, from aligned pointers and from pointers offset by an element.  No atomics, no
 * grid-wide synchronisation, nothing read back, no workspace beyond `part` and `state`.
 *
 * Before any launch: TTR_E_INVALID for a bad dtype, n < 1, step < 0, a null pointer, or two vectors of the call that share a
 * byte; TTR_E_WORKSPACE for workspace_bytes below ttr_cg_workspace_bytes; TTR_E_UNSUPPORTED for n of 2^57 or more.
 * Profiling kind: TTR_PROF_MISC.
 */
#define TTR_CG_MAX_PARTS 256
int ttr_cg_parts(int dtype, int64_t n);
int64_t ttr_cg_workspace_bytes(int dtype, int64_t n);
int ttr_cg_dot(int dtype, int64_t n, const void* p, const void* Bp, double* part, int64_t workspace_bytes, void* stream);
int ttr_cg_update(int dtype, int step, int64_t n, const void* p, const void* Bp, void* v, void* r, double* part,
                  int64_t workspace_bytes, double* state, void* stream);
int ttr_cg_direction(int dtype, int step, int64_t n, const void* r, void* p, const double* part, int64_t workspace_bytes,
                     double* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTROUND_HIP_H */
