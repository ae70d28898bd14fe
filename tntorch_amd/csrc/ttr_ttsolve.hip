// Half of a three-layer environment application (ttsolve.py `tt_solve`), for gfx950:
//   ttr_env_half_apply   H[r, i, a', s'] = sum_{a, j} G[a, i, j, a'] * ( sum_{r'} Phi[r, a, r'] * X[r', j, s'] )
//                        Phi [R, A, R'] (contiguous), X [R', J, S'] (3 element strides), G [A, I, J, A'] (4 element strides)
//                        -> H [R, I, A', S'] (contiguous)
// Phi is an interface of (bra, matrix, ket), G a TT-matrix core, X a ket core.  The layout of H is the point: the local matvec
// y[r, i, s] = sum_{a', s'} H[r, i, a', s'] Psi[s, a', s'] and the environment update Phi'[s, a', s'] = sum_{r, i} Y[r, i, s]
// H[r, i, a', s'] are both plain GEMMs on H as it lies.
//
// Two chained GEMMs.  Stage 1, for every k = (a, j) (k = a J + j): T_k [R, S'] = Phi[:, a, :] @ X[:, j, :], a sum over r'.
// Stage 2, for every r: H[r] [(i, a'), S'] = G2^T @ T[r], with G2 [(a, j), (i, a')] a strided view of G, a sum over k.  The
// intermediate T [R, A J, S'] is never stored: a workgroup (4 waves) owns kTR r x kTS s' x kTN columns n = (i, a') of H and walks k
// in chunks of kKC.  Per chunk
//   - the G2 chunk [kKC][kTN] is staged in LDS (each thread owns a column n: its (i, a') offset is computed once; (a, j) of a row
//     by one 32-bit division; loads are unconditional from clamped addresses, dead values zeroed afterwards),
//   - wave w computes the kTR x kTS tiles T_k of k = k0 + w, k0 + w + 4, ... (4 independent accumulators) on
//     v_mfma_{f32,f64}_16x16x4 with both operands straight from global memory (Phi: lanes along r, quads along r'; X: lanes along
//     s'; everything past R, R', S' or K is a zero; the loads of four quads of r' are in flight together, and the first four
//     quads of a chunk are loaded one chunk ahead, behind stage 2 of the chunk before, as is the G2 chunk) and writes them to
//     LDS [kk][r][s'],
//   - wave w multiplies the r = 4 w .. 4 w + 3 of the tile: A operand G2^T (lanes along n), B operand T[r] (lanes along s'), so
//     the accumulator has s' on the lanes and n in the registers and is stored from the registers, 16 consecutive s' per lane
//     group (consecutive n are S' apart: one run where S' = 16).
// What is recomputed: stage 1 once per column tile, 2 R R' A J S' ceil(I A' / kTN) flops next to stage 2's 2 R S' A J I A' -- the
// share R' / kTN of it (DESIGN section 29 for why that is the right trade at TT ranks).
//
// No workspace, no atomics, no split of either sum across workgroups.  An element of H is ONE chain: its T values are chains from
// 0 in increasing r' (quads, the tail zero-filled), and it is a chain from 0 in increasing k over them (quads inside chunks of kKC,
// the tail zero-filled or skipped): the bits depend on R', A, J and the dtype, not on the element's place in a tile or on the
// other extents.  Nothing is read out of bounds; global offsets are 64-bit.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int kTR = TTR_ENV_TILE_R, kTS = TTR_ENV_TILE_S, kTN = TTR_ENV_TILE_N, kKC = TTR_ENV_TILE_K;
static_assert(kTR == 16 && kTS == 16 && kTN == 64 && kKC == 16, "the wave split and the fragment maps are written for these tiles");
constexpr int kLdr = kTS + 4;           // T tile, one r: the 4 r a lane group writes (fp32: 4 apart) fall into disjoint banks
constexpr int kLdt = kTR * kLdr + 16;   // T tile, one k: the 4 (fp64: 2) k of an operand read fall into disjoint banks
constexpr int kLdg = kTN + 16;          // G tile, one k: likewise
constexpr int kPer = kKC / (kThreads / kWave);   // stage-1 tiles per wave and chunk
constexpr int kQ = 4;                            // quads of r' whose loads are in flight together

template <typename T>
struct EnvArgs {
  int64_t R, A, Rp, J, Sp, I, Ap;
  int64_t K, N;              // A J, I A': both below 2^31
  int64_t xs[3], gs[4];      // element strides of X and G
  int64_t ntiles, stiles;
  const T* Phi;
  const T* X;
  const T* G;
  T* H;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void env_half_apply_kernel(EnvArgs<T> p) {
  __shared__ T Ts[kKC * kLdt];
  __shared__ T Gs[kKC * kLdg];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), l15 = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  int64_t b = blockIdx.x;
  const int64_t nt = b % p.ntiles;
  b /= p.ntiles;
  const int64_t st = b % p.stiles, rt = b / p.stiles;
  const int64_t r0 = rt * kTR, s0 = st * kTS, n0 = nt * kTN;
  const int ncols = p.N - n0 < kTN ? (int)(p.N - n0) : kTN;   // live columns of this tile, >= 1
  const int ntl = (ncols + 15) / 16;
  int mlive = (int)(p.R - r0) - wave * 4;                      // live r of this wave in stage 2
  mlive = mlive < 0 ? 0 : (mlive > 4 ? 4 : mlive);

  // stage 1: this lane's row of Phi (r) and column of X (s')
  const bool r_ok = r0 + l15 < p.R, s_ok = s0 + l15 < p.Sp;
  const T* phi_row = p.Phi + (r_ok ? (r0 + l15) * p.A * p.Rp : 0);
  const T* x_col = p.X + (s_ok ? (s0 + l15) * p.xs[2] : 0);
  // G loader: this thread's column n = (i, a')
  const int gc = tid & 63;
  const bool g_ok = gc < ncols;
  int64_t gcol = 0;
  if (g_ok) {
    const uint32_t n = (uint32_t)(n0 + gc), i = n / (uint32_t)p.Ap;
    gcol = (int64_t)i * p.gs[1] + (int64_t)(n - i * (uint32_t)p.Ap) * p.gs[3];
  }

  typename Mfma<T>::Acc acc[4][kTN / 16];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int t = 0; t < kTN / 16; ++t) acc[m][t] = Mfma<T>::zero();

  // the G2 chunk of k0: this thread's kGPer elements, rows kk = it * 4 + tid / 64.  Loads are unconditional from clamped (valid)
  // addresses and the dead ones are zeroed afterwards: a load under a condition becomes a branch with a wait of its own
  constexpr int kGPer = kKC * kTN / kThreads;
  auto load_g = [&](int64_t k0, T* gv) {
#pragma unroll
    for (int it = 0; it < kGPer; ++it) {
      const int64_t k = k0 + it * (kThreads / kTN) + tid / kTN;
      const bool live = g_ok && k < p.K;
      const uint32_t kc = live ? (uint32_t)k : 0u, a = kc / (uint32_t)p.J, j = kc - a * (uint32_t)p.J;
      const T v = p.G[(int64_t)a * p.gs[0] + (int64_t)j * p.gs[2] + gcol];
      gv[it] = live ? v : T(0);
    }
  };
  T gv[kGPer];
  load_g(0, gv);

  // stage 1 works in passes of kQ quads of r': the 2 kQ kPer loads of a pass are issued together, unconditionally and from clamped
  // (valid) addresses, and the dead values are zeroed when the pass is multiplied.  The FIRST pass of a chunk is loaded one chunk
  // ahead, during stage 2 of the chunk before (for R' <= 4 kQ that is all of stage 1).
  auto k_of = [&](int64_t k0, int t, bool& ok, const T*& pa, const T*& px) {
    const int64_t k = k0 + wave + t * (kThreads / kWave);
    ok = k < p.K;
    const uint32_t kc = ok ? (uint32_t)k : 0u, a = kc / (uint32_t)p.J, j = kc - a * (uint32_t)p.J;
    pa = phi_row + (int64_t)a * p.Rp;
    px = x_col + (int64_t)j * p.xs[1];
  };
  auto load_pass = [&](int64_t k0, int64_t rq, T (&av)[kQ][kPer], T (&bv)[kQ][kPer]) {
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
      bool ok;
      const T* pa;
      const T* px;
      k_of(k0, t, ok, pa, px);
#pragma unroll
      for (int u = 0; u < kQ; ++u) {
        const int64_t rp = rq + 4 * u + lq, rc = rp < p.Rp ? rp : 0;
        av[u][t] = pa[rc];
        bv[u][t] = px[rc * p.xs[0]];
      }
    }
  };
  T pav[kQ][kPer], pbv[kQ][kPer];
  load_pass(0, 0, pav, pbv);

  for (int64_t k0 = 0; k0 < p.K; k0 += kKC) {
    // ---- G2 chunk: Gs[kk][n - n0] = G[a, i, j, a'], zeros past K or N (loaded during the previous chunk's stage 2)
#pragma unroll
    for (int it = 0; it < kGPer; ++it) Gs[(it * (kThreads / kTN) + tid / kTN) * kLdg + gc] = gv[it];
    // ---- stage 1: T_k = Phi[:, a, :] @ X[:, j, :] for this wave's k, one chain in increasing r' each
    typename Mfma<T>::Acc t1[kPer];
    bool k_ok[kPer];
#pragma unroll
    for (int t = 0; t < kPer; ++t) {
      k_ok[t] = k0 + wave + t * (kThreads / kWave) < p.K;
      t1[t] = Mfma<T>::zero();
    }
    auto mma_pass = [&](int64_t rq, T (&av)[kQ][kPer], T (&bv)[kQ][kPer]) {
#pragma unroll
      for (int u = 0; u < kQ; ++u)
        if (rq + 4 * u < p.Rp) {   // (uniform) a quad wholly past R' is skipped
          const bool rp_ok = rq + 4 * u + lq < p.Rp;
#pragma unroll
          for (int t = 0; t < kPer; ++t)
            t1[t] = Mfma<T>::mma((k_ok[t] && r_ok && rp_ok) ? av[u][t] : T(0), (k_ok[t] && s_ok && rp_ok) ? bv[u][t] : T(0), t1[t]);
        }
    };
    mma_pass(0, pav, pbv);
    for (int64_t rq = 4 * kQ; rq < p.Rp; rq += 4 * kQ) {
      T av[kQ][kPer], bv[kQ][kPer];
      load_pass(k0, rq, av, bv);
      mma_pass(rq, av, bv);
    }
#pragma unroll
    for (int t = 0; t < kPer; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        Ts[(wave + t * (kThreads / kWave)) * kLdt + Mfma<T>::row(lane, reg) * kLdr + l15] = t1[t][reg];
    __syncthreads();
    if (k0 + kKC < p.K) {   // in flight during stage 2
      load_g(k0 + kKC, gv);
      load_pass(k0 + kKC, 0, pav, pbv);
    }
    // ---- stage 2: H[r][n, s'] += G2^T[n, k] T[r][k, s'] for the wave's r, one chain in increasing k
    const int klive = p.K - k0 < kKC ? (int)(p.K - k0) : kKC;
    const int quads = (klive + 3) / 4;
    const T* g_row = Gs + lq * kLdg + l15;
    const T* t_col = Ts + lq * kLdt + wave * 4 * kLdr + l15;
    for (int q = 0; q < quads; ++q) {
      T g[kTN / 16], tt[4];
#pragma unroll
      for (int t = 0; t < kTN / 16; ++t) g[t] = g_row[q * 4 * kLdg + t * 16];
#pragma unroll
      for (int m = 0; m < 4; ++m) tt[m] = t_col[q * 4 * kLdt + m * kLdr];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int t = 0; t < kTN / 16; ++t)
          if (m < mlive && t < ntl) acc[m][t] = Mfma<T>::mma(g[t], tt[m], acc[m][t]);
    }
    __syncthreads();   // (the next chunk overwrites Ts / Gs)
  }

  // ---- store: lane holds s' = s0 + (lane & 15) of the columns n = 16 t + Mfma<T>::row(lane, 0 .. 3), for each of the wave's r
  if (s_ok) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (m < mlive) {
        T* h = p.H + (r0 + wave * 4 + m) * p.N * p.Sp + s0 + l15;
#pragma unroll
        for (int t = 0; t < kTN / 16; ++t)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int n = t * 16 + Mfma<T>::row(lane, reg);
            if (n < ncols) h[(n0 + n) * p.Sp] = acc[m][t][reg];
          }
      }
    }
  }
}

template <typename T>
int env_impl(EnvArgs<T> p, hipStream_t stream) {
  const int64_t rtiles = ceil_div(p.R, kTR);
  p.stiles = ceil_div(p.Sp, kTS);
  p.ntiles = ceil_div(p.N, kTN);
  const double blocks = (double)rtiles * (double)p.stiles * (double)p.ntiles;
  TTR_REQUIRE(blocks <= 2147483647.0, TTR_E_UNSUPPORTED, "ttr_env_half_apply: %.0f workgroups do not fit a 32-bit grid", blocks);
  ProfScope prof(TTR_PROF_GEMM, stream);
  hipLaunchKernelGGL((env_half_apply_kernel<T>), dim3((unsigned)(rtiles * p.stiles * p.ntiles)), dim3(kThreads), 0, stream, p);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

// no negative stride on a live axis, and the farthest element below 2^57 (the stride of an extent-1 axis is free)
inline bool strides_ok(const int64_t* shape, const int64_t* strides, int nd) {
  double far = 0.0;
  for (int d = 0; d < nd; ++d) {
    if (shape[d] == 1) continue;
    if (strides[d] < 0) return false;
    far += (double)(shape[d] - 1) * (double)strides[d];
  }
  return far < 9.0e18 / 64.0;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_env_half_apply(int dtype, int64_t R, int64_t A, int64_t Rp, int64_t J, int64_t Sp, int64_t I, int64_t Ap,
                                  const void* Phi, const void* X, const int64_t* x_strides, const void* G, const int64_t* g_strides,
                                  void* H, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_env_half_apply: bad dtype %d", dtype);
  TTR_REQUIRE(R >= 1 && A >= 1 && Rp >= 1 && J >= 1 && Sp >= 1 && I >= 1 && Ap >= 1, TTR_E_INVALID,
              "ttr_env_half_apply: bad sizes Phi [%lld, %lld, %lld], X [%lld, %lld, %lld], G [%lld, %lld, %lld, %lld]", (long long)R,
              (long long)A, (long long)Rp, (long long)Rp, (long long)J, (long long)Sp, (long long)A, (long long)I, (long long)J,
              (long long)Ap);
  TTR_REQUIRE(Phi && X && x_strides && G && g_strides && H, TTR_E_INVALID, "ttr_env_half_apply: null pointer");
  TTR_REQUIRE(H != Phi && H != X && H != G, TTR_E_INVALID, "ttr_env_half_apply: H must not be an input");
  const int64_t lim = 2147483647LL;
  TTR_REQUIRE(R <= lim && A <= lim && Rp <= lim && J <= lim && Sp <= lim && I <= lim && Ap <= lim, TTR_E_UNSUPPORTED,
              "ttr_env_half_apply: an extent does not fit 32 bits");
  TTR_REQUIRE(A * J <= lim && I * Ap <= lim, TTR_E_UNSUPPORTED, "ttr_env_half_apply: A J and I A' must be at most 2^31 - 1");
  const double big = 9.0e18 / 64.0;
  TTR_REQUIRE((double)R * (double)A * (double)Rp < big && (double)R * (double)I * (double)Ap * (double)Sp < big, TTR_E_UNSUPPORTED,
              "ttr_env_half_apply: operand too large");
  const int64_t xsh[3] = {Rp, J, Sp}, gsh[4] = {A, I, J, Ap};
  TTR_REQUIRE(strides_ok(xsh, x_strides, 3), TTR_E_UNSUPPORTED,
              "ttr_env_half_apply: X [R', J, S'] needs non-negative element strides that span less than 2^57 elements");
  TTR_REQUIRE(strides_ok(gsh, g_strides, 4), TTR_E_UNSUPPORTED,
              "ttr_env_half_apply: G [A, I, J, A'] needs non-negative element strides that span less than 2^57 elements");
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    EnvArgs<T> p{};
    p.R = R, p.A = A, p.Rp = Rp, p.J = J, p.Sp = Sp, p.I = I, p.Ap = Ap;
    p.K = A * J, p.N = I * Ap;
    for (int d = 0; d < 3; ++d) p.xs[d] = xsh[d] == 1 ? 0 : x_strides[d];
    for (int d = 0; d < 4; ++d) p.gs[d] = gsh[d] == 1 ? 0 : g_strides[d];
    p.Phi = (const T*)Phi, p.X = (const T*)X, p.G = (const T*)G, p.H = (T*)H;
    return env_impl<T>(p, (hipStream_t)stream);
  });
}
