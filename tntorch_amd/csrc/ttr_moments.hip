// Contractions of the TT moment family (metrics.py:345-455, `hadamard_sum`) on MFMA 16x16x4 (gfx950):
//   ttr_core_matvec  TT-matrix core x TT-vector core, written in the Kronecker-interleaved layout of the result
//   ttr_hsum_step    one mode of the exact K-way chain: K mode products, the sum over the mode index folded into the last
// Both are instances of ONE tile kernel, a batched product whose batch, column and contraction indices may each be a PAIR of
// tensor indices (index = hi * div + lo, one element stride per part and tensor):
//   C[b][m][n] = sum_k X[b][m][k] * Y[b][n][k]
// so a core is read where it lies ([a, k, s, c] / [r, i, r']) and the result is written where it belongs: no operand is
// permuted, repeated or copied, and there is no un-permuted intermediate.  The tile is ttr_gemm's small-product tile (four
// waves, 32 x 32 of C per wave, K walked in steps of 16 through LDS, global loads of the next step in flight under the MFMAs);
// the LDS image of either operand is [k][mn]: in every use here the mn index of at least one operand is the unit-stride axis,
// and consecutive threads stage consecutive mn.  Every global read and write is guarded by its extent (ragged tiles are zero
// filled), and every extent and stride comes from validated host arguments.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int MBK = 16;  // K step
constexpr int MPAD = 16;

template <typename T>
struct ConArgs {
  int64_t M, N, K;
  int64_t bdiv, ndiv, kdiv;  // batch / column / contraction index = hi * div + lo   (div = 0: lo only)
  const T* X; int64_t x_bh, x_bl, x_m, x_kh, x_kl;
  const T* Y; int64_t y_bh, y_bl, y_nh, y_nl, y_kh, y_kl;
  T* C; int64_t c_bh, c_bl, c_m, c_nh, c_nl;
  int tilesN;
  int64_t b0;  // first batch item of this launch (the batch is a grid dimension: long batches run in slices)
};

template <typename T, int BM, int BN, int WN>
__global__ __launch_bounds__(kThreads) void contract_kernel(ConArgs<T> p) {
  constexpr int EA = BM * MBK / kThreads, EB = BN * MBK / kThreads;  // staged elements per thread and K step
  constexpr int LDA = BM + MPAD, LDB = BN + MPAD;
  __shared__ T As[MBK * LDA];
  __shared__ T Bs[MBK * LDB];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int64_t b = p.b0 + blockIdx.z;
  const int64_t bh = p.bdiv ? b / p.bdiv : 0, bl = p.bdiv ? b % p.bdiv : b;
  const int64_t m0 = (int64_t)(blockIdx.x / p.tilesN) * BM;
  const int64_t n0 = (int64_t)(blockIdx.x % p.tilesN) * BN;

  const T* __restrict__ X = p.X + bh * p.x_bh + bl * p.x_bl;
  const T* __restrict__ Y = p.Y + bh * p.y_bh + bl * p.y_bl;

  // per-thread staging coordinates: consecutive threads take consecutive mn of one k
  int ai[EA], ak[EA], bj[EB], bk[EB];
  int64_t aoff[EA], boff[EB];
  bool aok[EA], bok[EB];
#pragma unroll
  for (int e = 0; e < EA; ++e) {
    const int idx = tid + kThreads * e;
    ai[e] = idx % BM; ak[e] = idx / BM;
    const int64_t gi = m0 + ai[e];
    aok[e] = gi < p.M;
    aoff[e] = gi * p.x_m;
  }
#pragma unroll
  for (int e = 0; e < EB; ++e) {
    const int idx = tid + kThreads * e;
    bj[e] = idx % BN; bk[e] = idx / BN;
    const int64_t gj = n0 + bj[e];
    bok[e] = gj < p.N;
    const int64_t nh = p.ndiv ? gj / p.ndiv : 0, nl = p.ndiv ? gj % p.ndiv : gj;
    boff[e] = nh * p.y_nh + nl * p.y_nl;
  }

  typename Mfma<T>::Acc acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = Mfma<T>::zero();

  T ra[EA], rb[EB];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int e = 0; e < EA; ++e) {
      const int64_t gk = k0 + ak[e];
      const int64_t kh = p.kdiv ? gk / p.kdiv : 0, kl = p.kdiv ? gk % p.kdiv : gk;
      ra[e] = (aok[e] && gk < p.K) ? X[aoff[e] + kh * p.x_kh + kl * p.x_kl] : T(0);
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      const int64_t gk = k0 + bk[e];
      const int64_t kh = p.kdiv ? gk / p.kdiv : 0, kl = p.kdiv ? gk % p.kdiv : gk;
      rb[e] = (bok[e] && gk < p.K) ? Y[boff[e] + kh * p.y_kh + kl * p.y_kl] : T(0);
    }
  };

  fetch(0);
  for (int64_t k0 = 0; k0 < p.K; k0 += MBK) {
#pragma unroll
    for (int e = 0; e < EA; ++e) As[ak[e] * LDA + ai[e]] = ra[e];
#pragma unroll
    for (int e = 0; e < EB; ++e) Bs[bk[e] * LDB + bj[e]] = rb[e];
    __syncthreads();
    if (k0 + MBK < p.K) fetch(k0 + MBK);  // overlaps the MFMAs below
#pragma unroll
    for (int kk = 0; kk < MBK / 4; ++kk) {
      const int kf = kk * 4 + (lane >> 4);
      T a[2], bb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = As[kf * LDA + wm * 32 + t * 16 + (lane & 15)];
        bb[t] = Bs[kf * LDB + wn * 32 + t * 16 + (lane & 15)];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = Mfma<T>::mma(a[i], bb[j], acc[i][j]);
    }
    __syncthreads();
  }

  T* __restrict__ C = p.C + bh * p.c_bh + bl * p.c_bl;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t col = n0 + wn * 32 + j * 16 + (lane & 15);
    if (col >= p.N) continue;
    const int64_t nh = p.ndiv ? col / p.ndiv : 0, nl = p.ndiv ? col % p.ndiv : col;
    T* __restrict__ Cc = C + nh * p.c_nh + nl * p.c_nl;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + wm * 32 + i * 16 + Mfma<T>::row(lane, r);
        if (row < p.M) Cc[row * p.c_m] = acc[i][j][r];
      }
  }
}

// tile shapes as in ttr_gemm: 64 x 64, or 128 x 32 / 32 x 128 when one side has at most 32 entries
template <typename T>
int contract_launch(ConArgs<T> p, int64_t batch, hipStream_t stream, const char* who) {
  TTR_REQUIRE(p.M <= 2147483647LL && p.N <= 2147483647LL && p.K <= 2147483647LL, TTR_E_UNSUPPORTED, "%s: extent above 2^31 - 1", who);
  const int shape = (p.N <= 32 && p.M >= 128) ? 1 : ((p.M <= 32 && p.N >= 128) ? 2 : 0);
  const int64_t BM = shape == 1 ? 128 : (shape == 2 ? 32 : 64), BN = shape == 1 ? 32 : (shape == 2 ? 128 : 64);
  const int64_t tilesM = ceil_div(p.M, BM), tilesN = ceil_div(p.N, BN);
  TTR_REQUIRE(tilesM * tilesN <= 2147483647LL, TTR_E_UNSUPPORTED, "%s: too many tiles", who);
  p.tilesN = (int)tilesN;
  ProfScope prof(TTR_PROF_MISC, stream);
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
    p.b0 = b0;
    const dim3 grid((unsigned)(tilesM * tilesN), 1, (unsigned)nb);
    if (shape == 1)
      hipLaunchKernelGGL((contract_kernel<T, 128, 32, 1>), grid, dim3(kThreads), 0, stream, p);
    else if (shape == 2)
      hipLaunchKernelGGL((contract_kernel<T, 32, 128, 4>), grid, dim3(kThreads), 0, stream, p);
    else
      hipLaunchKernelGGL((contract_kernel<T, 64, 64, 2>), grid, dim3(kThreads), 0, stream, p);
  }
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

// out[p A + a, s, q C + c] = sum_k x[p, k, q] G[a, k, s, c]: batch (p, s), rows q, columns (a, c)
template <typename T>
int core_matvec_impl(int64_t P, int64_t K, int64_t Q, int64_t A, int64_t S, int64_t C, const void* x, const void* G, void* out,
                     hipStream_t stream) {
  ConArgs<T> p{};
  p.M = Q; p.N = A * C; p.K = K;
  p.bdiv = S; p.ndiv = C; p.kdiv = 0;
  p.X = (const T*)x; p.x_bh = K * Q; p.x_bl = 0; p.x_m = 1; p.x_kh = 0; p.x_kl = Q;
  p.Y = (const T*)G; p.y_bh = 0; p.y_bl = C; p.y_nh = K * S * C; p.y_nl = 1; p.y_kh = 0; p.y_kl = S * C;
  p.C = (T*)out; p.c_bh = A * S * Q * C; p.c_bl = Q * C; p.c_m = C; p.c_nh = S * Q * C; p.c_nl = 1;
  return contract_launch<T>(p, P * S, stream, "ttr_core_matvec");
}

constexpr int64_t kHsumMaxK = 8;
constexpr int64_t kHsumMaxScratch = 1LL << 32;  // bytes

// extents of the K - 1 intermediates T_m [I, r'_1 .. r'_m, r_{m+1} .. r_K]; returns the largest element count (0 for K = 1),
// -1 when a product leaves the envelope
int64_t hsum_max_elems(int64_t K, int64_t I, const int64_t* rin, const int64_t* rout) {
  const double lim = 4.0e18;
  int64_t mx = 0;
  for (int64_t m = 0; m + 1 < K; ++m) {
    double d = (double)I;
    int64_t e = I;
    for (int64_t j = 0; j < K; ++j) {
      const int64_t f = j <= m ? rout[j] : rin[j];
      d *= (double)f;
      if (d > lim) return -1;
      e *= f;
    }
    if (e > mx) mx = e;
  }
  return mx;
}

template <typename T>
int hsum_step_impl(int64_t K, int64_t I, const int64_t* rin, const int64_t* rout, const void* W, const void* const* cores,
                   void* Wout, void* ws, hipStream_t stream) {
  const int64_t half = align_up(hsum_max_elems(K, I, rin, rout) * (int64_t)sizeof(T), 256);
  T* buf[2] = {(T*)ws, (T*)((char*)ws + half)};
  const T* cur = (const T*)W;
  int64_t L = 1;
  for (int64_t m = 0; m + 1 < K; ++m) {  // T_m[i, l, a', rt] = sum_a A_m[a, i, a'] T_{m-1}[i, l, a, rt]   (T_{-1} = W for every i)
    int64_t Rt = 1;
    for (int64_t j = m + 1; j < K; ++j) Rt *= rin[j];
    const int64_t r = rin[m], rp = rout[m];
    ConArgs<T> p{};
    p.M = rp; p.N = Rt; p.K = r;
    p.bdiv = L; p.ndiv = 0; p.kdiv = 0;
    p.X = (const T*)cores[m]; p.x_bh = rp; p.x_bl = 0; p.x_m = 1; p.x_kl = I * rp;
    p.Y = cur; p.y_bh = m == 0 ? 0 : L * r * Rt; p.y_bl = r * Rt; p.y_nl = 1; p.y_kl = Rt;
    p.C = buf[m & 1]; p.c_bh = L * rp * Rt; p.c_bl = rp * Rt; p.c_m = Rt; p.c_nl = 1;
    const int rc = contract_launch<T>(p, I * L, stream, "ttr_hsum_step");
    if (rc != TTR_OK) return rc;
    cur = buf[m & 1];
    L *= rp;
  }
  // W'[l, a'] = sum_{i, a} T_{K-2}[i, l, a] A_K[a, i, a']: the sum over i rides in the contraction index (i, a)
  const int64_t r = rin[K - 1], rp = rout[K - 1];
  ConArgs<T> p{};
  p.M = L; p.N = rp; p.K = I * r;
  p.bdiv = 0; p.ndiv = 0; p.kdiv = r;
  p.X = cur; p.x_m = r; p.x_kh = K == 1 ? 0 : L * r; p.x_kl = 1;
  p.Y = (const T*)cores[K - 1]; p.y_nl = 1; p.y_kh = rp; p.y_kl = I * rp;
  p.C = (T*)Wout; p.c_m = rp; p.c_nl = 1;
  return contract_launch<T>(p, 1, stream, "ttr_hsum_step");
}

int hsum_check(int dtype, int64_t K, int64_t I, const int64_t* rin, const int64_t* rout) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_hsum_step: bad dtype %d", dtype);
  TTR_REQUIRE(K >= 1 && I >= 1 && rin && rout, TTR_E_INVALID, "ttr_hsum_step: bad sizes");
  TTR_REQUIRE(K <= kHsumMaxK, TTR_E_UNSUPPORTED, "ttr_hsum_step: K = %lld > %lld", (long long)K, (long long)kHsumMaxK);
  double win = 1.0, wout = 1.0;
  for (int64_t m = 0; m < K; ++m) {
    TTR_REQUIRE(rin[m] >= 1 && rout[m] >= 1, TTR_E_INVALID, "ttr_hsum_step: rank < 1");
    TTR_REQUIRE(rin[m] <= 2147483647LL / I && rout[m] <= 2147483647LL / I, TTR_E_UNSUPPORTED, "ttr_hsum_step: core too large");
    win *= (double)rin[m]; wout *= (double)rout[m];
  }
  TTR_REQUIRE(win <= 2147483647.0 && wout <= 2147483647.0, TTR_E_UNSUPPORTED, "ttr_hsum_step: prod(ranks) above 2^31 - 1");
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_core_matvec(int dtype, int64_t P, int64_t K, int64_t Q, int64_t A, int64_t S, int64_t C, const void* x,
                               const int64_t* x_strides, const void* G, const int64_t* g_strides, void* out, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_core_matvec: bad dtype %d", dtype);
  TTR_REQUIRE(P >= 1 && K >= 1 && Q >= 1 && A >= 1 && S >= 1 && C >= 1, TTR_E_INVALID, "ttr_core_matvec: bad sizes");
  TTR_REQUIRE(x && G && out && x_strides && g_strides, TTR_E_INVALID, "ttr_core_matvec: null pointer");
  const int64_t xs[3] = {P, K, Q}, gs[4] = {A, K, S, C};
  TTR_REQUIRE(contiguous(xs, x_strides, 3) && contiguous(gs, g_strides, 4), TTR_E_UNSUPPORTED,
              "ttr_core_matvec: x and G must be contiguous");
  const double lim = 9.0e18 / 8.0;
  TTR_REQUIRE((double)P * (double)A * (double)S * (double)Q * (double)C < lim && (double)A * (double)K * (double)S * (double)C < lim &&
                  (double)P * (double)K * (double)Q < lim && A <= 2147483647LL / C && P <= 2147483647LL / S,
              TTR_E_UNSUPPORTED, "ttr_core_matvec: core too large");
  return by_dtype(dtype, [&](auto t) { return core_matvec_impl<decltype(t)>(P, K, Q, A, S, C, x, G, out, (hipStream_t)stream); });
}

extern "C" int64_t ttr_hsum_step_workspace_bytes(int dtype, int64_t K, int64_t I, const int64_t* r_in, const int64_t* r_out) {
  const int rc = hsum_check(dtype, K, I, r_in, r_out);
  if (rc != TTR_OK) return rc;
  const int64_t mx = hsum_max_elems(K, I, r_in, r_out);
  const int64_t elem = elem_size(dtype);
  TTR_REQUIRE(mx >= 0 && mx <= kHsumMaxScratch / (2 * elem), TTR_E_UNSUPPORTED,
              "ttr_hsum_step: the intermediates of these ranks need more than %lld bytes of scratch", (long long)kHsumMaxScratch);
  return 2 * align_up(mx * elem, 256);
}

extern "C" int ttr_hsum_step(int dtype, int64_t K, int64_t I, const int64_t* r_in, const int64_t* r_out, const void* W,
                             const void* const* cores, const int64_t* core_strides, void* Wout, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  const int64_t need = ttr_hsum_step_workspace_bytes(dtype, K, I, r_in, r_out);
  if (need < 0) return (int)need;
  TTR_REQUIRE(W && cores && core_strides && Wout, TTR_E_INVALID, "ttr_hsum_step: null pointer");
  for (int64_t m = 0; m < K; ++m) {
    TTR_REQUIRE(cores[m], TTR_E_INVALID, "ttr_hsum_step: null core %lld", (long long)m);
    const int64_t cs[3] = {r_in[m], I, r_out[m]};
    TTR_REQUIRE(contiguous(cs, core_strides + 3 * m, 3), TTR_E_UNSUPPORTED, "ttr_hsum_step: core %lld is not contiguous", (long long)m);
  }
  TTR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), TTR_E_WORKSPACE, "ttr_hsum_step: workspace %lld < %lld bytes",
              (long long)workspace_bytes, (long long)need);
  return by_dtype(dtype, [&](auto t) { return hsum_step_impl<decltype(t)>(K, I, r_in, r_out, W, cores, Wout, workspace, (hipStream_t)stream); });
}
