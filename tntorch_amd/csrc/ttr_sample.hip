// One mode of drawing P index vectors from a train read as an unnormalised mass function (tools.py:362-407 `sample`: a P x I
// matrix lefts @ fiber, then abs, a row normalisation, hstack, cumsum, a subtraction and a sign test, about ten passes over it).
// Here the matrix never exists: per sample p, with q[i] = |L[p, :] . fiber[:, i]| in the dtype,
//   T = sum_i q[i] (fp64 running sum c_i), x = the smallest i with c_i > u T, Lnew[p, :] = (L[p, :] @ core[:, x, :]) / T.
//
// Tiling.  A wave owns NS samples (32 in fp32, 16 in fp64), a workgroup of four waves S = 4 NS of them (TTR_SAMPLE_TILE_*).  The
// wave's rows of L are staged once in LDS ([NS, r] padded with zeros to a multiple of four MFMA steps, odd row stride).  q is formed one block of
// B = NS columns of fiber at a time (TTR_SAMPLE_BLOCK_*) on the matrix cores, D = A B with A = the block of fiber transposed
// (row = column of fiber, from global memory: every wave of the grid reads the same r x I matrix, it stays in cache) and B = the
// rows of L transposed (column = sample, from LDS): v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, r / 2 or r / 4 per block.
// The rows of A are PERMUTED so that the results a lane holds are CONSECUTIVE columns of its sample: in fp32 the lane pair
// (j, j + 32) of sample j holds columns [c0, c0 + 16) and [c0 + 16, c0 + 32) in register order, in fp64 the four lanes
// j + 16 g hold [c0 + 4 g, c0 + 4 g + 4).  A lane sums its segment in fp64 in column order, the segment sums are exchanged between
// the lanes of the sample, and the running sum at a segment's first column is the running sum of the block's start plus the
// earlier segments, added in order.  c_i is therefore one fixed, non-decreasing fp64 sequence per sample, and no reduction crosses
// samples.
//
// Two passes over the blocks, both on the matrix cores and forming the same q: the first leaves T (in fp64 dtype a compensated
// sum, so that T and c_{I-1} may differ in the last place; the rule for "no crossing" covers it), the second finds the first
// c_i > u T (the in-lane scan runs only in the block where the running sum crosses u T) and the last i with q[i] > 0 (taken when
// rounding of u T leaves no crossing).  Block totals kept in LDS would save the second pass for I up to a few thousand and cap I;
// this form has no limit on I, its LDS does not depend on I, and it still moves r I elements of fiber (cached) per pass instead of
// P I of the matrix.  The first i with c_i > u T always has q[i] > 0: c_i > c_{i-1} there.
//
// Update: lanes run over (sample, column of Lnew), a loop over r with L[p, a] from LDS and core[a, x, b] gathered (consecutive
// lanes read consecutive b); fma chain in the dtype, the quotient by T in fp64, one rounding at the store.
//
// Bounds: every store is indexed by the sample's own p < P (X[p stride_x], Lnew[p ldn + b], b < rn); rows of the tile beyond P are
// staged as zeros and store nothing.  The only data-dependent address is the LOAD of core[:, x, :] with 0 <= x < I: x is a column
// the scan visited, and columns >= I are masked to q = 0 at the load and cannot be chosen.  A flagged sample (T zero or not
// finite, u outside [0, 1)) stores X = -1 and a zero row and loads nothing from core.  The word is ORed with one vector atomic
// per flagged sample.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int kMaxRank = 128;  // LDS: 4 NS rows of kMaxRank + 1 elements = 66048 bytes in either dtype

constexpr int kUnroll = 4;     // MFMA steps per trip of the K loop; r is padded to kUnroll K

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <typename T>
struct Tile;

template <>
struct Tile<float> {
  static constexpr int NS = 32;   // samples per wave = columns per block
  static constexpr int KS = 2;    // K of the MFMA
  static constexpr int SEG = 16;  // consecutive columns per lane
  using Acc = f32x16;
  static __device__ __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
  // C/D row m = 8 (reg >> 2) + 4 (lane >> 5) + (reg & 3): row m of A is column 16 h + 4 a + b for m = 8 a + 4 h + b
  static __device__ __forceinline__ int perm(int m) { return 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3); }
};

template <>
struct Tile<double> {
  static constexpr int NS = 16;
  static constexpr int KS = 4;
  static constexpr int SEG = 4;
  using Acc = f64x4;
  static __device__ __forceinline__ Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  // C/D row m = (lane >> 4) + 4 reg: row m of A is column 4 (m & 3) + (m >> 2)
  static __device__ __forceinline__ int perm(int m) { return 4 * (m & 3) + (m >> 2); }
};

static_assert(4 * Tile<float>::NS == TTR_SAMPLE_TILE_F32 && 4 * Tile<double>::NS == TTR_SAMPLE_TILE_F64, "header and kernel disagree");
static_assert(Tile<float>::NS == TTR_SAMPLE_BLOCK_F32 && Tile<double>::NS == TTR_SAMPLE_BLOCK_F64, "header and kernel disagree");

template <typename T>
struct SampleArgs {
  int64_t P, r, I, rn;
  const T* L;
  int64_t ldl;
  const T* fiber;
  const T* core;
  int64_t cs0, cs1, cs2;
  const double* u;
  int64_t stride_u;
  int64_t* X;
  int64_t stride_x;
  T* Lnew;  // null at the last mode
  int64_t ldn;
  int* flag;
  int rp, lds;  // r rounded up to kUnroll KS; the row stride of the staged rows (odd)
};

// q of one block for this lane's sample: SEG consecutive columns from c0 + SEG * (lane / NS), as fp64
template <typename T>
__device__ __forceinline__ void form_block(const SampleArgs<T>& a, const T* Lrow, int64_t c0, int lane, double (&q)[Tile<T>::SEG]) {
  using Tl = Tile<T>;
  const int g = lane / Tl::NS;
  const int64_t col = c0 + Tl::perm(lane % Tl::NS);
  const bool cok = col < a.I;
  const T* fp = a.fiber + (cok ? col : 0);
  typename Tl::Acc acc;
#pragma unroll
  for (int t = 0; t < Tl::SEG; ++t) acc[t] = T(0);
  for (int k0 = 0; k0 < a.rp; k0 += kUnroll * Tl::KS) {  // the loads of kUnroll steps in flight before their MFMAs
    T av[kUnroll], bv[kUnroll];
#pragma unroll
    for (int v = 0; v < kUnroll; ++v) {
      const int k = k0 + v * Tl::KS + g;
      av[v] = (cok && k < a.r) ? fp[(int64_t)k * a.I] : T(0);
      bv[v] = Lrow[k];
    }
#pragma unroll
    for (int v = 0; v < kUnroll; ++v) acc = Tl::mma(av[v], bv[v], acc);
  }
#pragma unroll
  for (int t = 0; t < Tl::SEG; ++t) q[t] = fabs((double)acc[t]);
}

// s + c <- s + c + x with s + x rounded once and what the rounding lost added to c (Knuth's two-sum; NaN and infinity pass into s)
__device__ __forceinline__ void two_sum(double& s, double& c, double x) {
  const double t = s + x, bp = t - s;
  c += (s - (t - bp)) + (x - bp);
  s = t;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void sample_step_kernel(SampleArgs<T> a) {
  using Tl = Tile<T>;
  constexpr int NS = Tl::NS, SEG = Tl::SEG, NG = kWave / NS;
  extern __shared__ double sample_smem[];
  __shared__ int x_sh[kThreads / kWave][NS];
  __shared__ double t_sh[kThreads / kWave][NS];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane % NS, g = lane / NS;
  const int64_t p0 = ((int64_t)blockIdx.x * (kThreads / kWave) + wave) * NS;  // the wave's first sample
  T* Lw = (T*)sample_smem + (int64_t)wave * NS * a.lds;

  for (int idx = lane; idx < NS * a.rp; idx += kWave) {
    const int s = idx / a.rp, k = idx - s * a.rp;
    Lw[s * a.lds + k] = (p0 + s < a.P && k < a.r) ? a.L[(p0 + s) * a.ldl + k] : T(0);
  }
  __syncthreads();

  const int64_t p = p0 + j;
  const bool live = p < a.P;
  const T* Lrow = Lw + j * a.lds;
  const int64_t Iw = p0 < a.P ? a.I : 0;  // a wave with no sample of its own forms nothing
  double q[SEG];

  // pass 1: T.  Every lane adds up its own columns (in fp64 dtype with the rounding of each addition carried along: T is then
  // good to an ulp, as the quotient of the update needs it; in fp32 the plain fp64 sum is already 2^29 times finer than q),
  // then the lanes of a sample add their parts in one fixed order.
  double sum = 0.0, carry = 0.0;
  for (int64_t c0 = 0; c0 < Iw; c0 += NS) {
    form_block<T>(a, Lrow, c0, lane, q);
#pragma unroll
    for (int t = 0; t < SEG; ++t) {
      if (sizeof(T) == 8) two_sum(sum, carry, q[t]);
      else sum += q[t];
    }
  }
  double total = 0.0, tcarry = 0.0;
#pragma unroll
  for (int h = 0; h < NG; ++h) {
    two_sum(total, tcarry, __shfl(sum, j + NS * h, kWave));
    tcarry += __shfl(carry, j + NS * h, kWave);
  }
  total += tcarry;
  const double uu = live ? a.u[p * a.stride_u] : 0.0;
  int bits = 0;
  if (!(uu >= 0.0 && uu < 1.0)) bits |= TTR_SAMPLE_BAD_THRESHOLD;
  if (total == 0.0) bits |= TTR_SAMPLE_ZERO_TOTAL;
  else if (!(total > 0.0 && total < INFINITY)) bits |= TTR_SAMPLE_NONFINITE;
  const double thr = uu * total;

  // pass 2: the same running sum again; first column with c > thr, last column with q > 0
  int first = 0x7fffffff, last = -1;
  double run = 0.0;
  for (int64_t c0 = 0; c0 < Iw; c0 += NS) {
    form_block<T>(a, Lrow, c0, lane, q);
    double seg = q[0];
#pragma unroll
    for (int t = 1; t < SEG; ++t) seg += q[t];
    const double start = run;
    double base = run;  // the running sum before this lane's segment
#pragma unroll
    for (int h = 0; h < NG; ++h) {
      const double sh = __shfl(seg, j + NS * h, kWave);
      run += sh;
      if (h < g) base += sh;
    }
    const int col0 = (int)c0 + SEG * g;
#pragma unroll
    for (int t = 0; t < SEG; ++t)
      if (q[t] > 0.0) last = col0 + t;
    if (first == 0x7fffffff && !(start > thr) && run > thr) {
      double part = 0.0;
#pragma unroll
      for (int t = 0; t < SEG; ++t) {
        part += q[t];
        if (first == 0x7fffffff && base + part > thr) first = col0 + t;
      }
    }
  }
#pragma unroll
  for (int h = 1; h < NG; ++h) {  // the lanes of a sample agree: the smallest crossing, the largest column of positive mass
    const int f2 = __shfl_xor(first, NS * h, kWave), l2 = __shfl_xor(last, NS * h, kWave);
    first = f2 < first ? f2 : first;
    last = l2 > last ? l2 : last;
  }
  int x = first != 0x7fffffff ? first : last;
  if (bits || x < 0 || x >= a.I) x = -1;  // (neither can happen without a flag: a positive T has a column of positive mass, and
                                          // the masked columns >= I have none)
  if (g == 0) {
    x_sh[wave][j] = x;
    t_sh[wave][j] = total;
    if (live) {
      a.X[p * a.stride_x] = x;
      if (bits) atomicOr(a.flag, bits);
    }
  }
  if (!a.Lnew) return;
  __syncthreads();

  const int rn = (int)a.rn;
  for (int idx = lane; idx < NS * rn; idx += kWave) {
    const int s = idx / rn, b = idx - s * rn;
    if (p0 + s >= a.P) break;  // idx grows with s: nothing further is live
    const int xs = x_sh[wave][s];
    T out = T(0);
    if (xs >= 0) {
      const T* cp = a.core + (int64_t)xs * a.cs1 + (int64_t)b * a.cs2;
      const T* lr = Lw + s * a.lds;
      T acc = T(0);
      for (int k = 0; k < (int)a.r; ++k) acc = fma(lr[k], cp[(int64_t)k * a.cs0], acc);
      out = (T)((double)acc / t_sh[wave][s]);
    }
    a.Lnew[(p0 + s) * a.ldn + b] = out;
  }
}

template <typename T>
int sample_impl(SampleArgs<T> a, hipStream_t stream) {
  using Tl = Tile<T>;
  ProfScope prof(TTR_PROF_MISC, stream);
  a.rp = (int)align_up(a.r, kUnroll * Tl::KS);
  a.lds = a.rp | 1;
  const size_t lds = (size_t)(kThreads / kWave) * Tl::NS * a.lds * sizeof(T);
  auto kern = sample_step_kernel<T>;
  if (lds > 64 * 1024) TTR_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t blocks = ceil_div(a.P, (int64_t)(kThreads / kWave) * Tl::NS);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kThreads), lds, stream, a);
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_sample_max_rank(void) { return kMaxRank; }

extern "C" int ttr_sample_step(int dtype, int64_t P, int64_t r, int64_t I, int64_t rn, const void* L, int64_t ldl, const void* fiber,
                               const void* core, const int64_t* core_strides, const void* u, int64_t stride_u, void* X,
                               int64_t stride_x, void* Lnew, int64_t ldn, void* flag, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_sample_step: bad dtype %d", dtype);
  TTR_REQUIRE(P >= 0 && r >= 1 && I >= 1 && rn >= 1, TTR_E_INVALID, "ttr_sample_step: bad sizes P = %lld, core [%lld, %lld, %lld]",
              (long long)P, (long long)r, (long long)I, (long long)rn);
  TTR_REQUIRE(r <= kMaxRank && rn <= kMaxRank, TTR_E_INVALID,
              "ttr_sample_step: ranks %lld, %lld above the limit of %d (ttr_sample_max_rank)", (long long)r, (long long)rn, kMaxRank);
  TTR_REQUIRE(L && fiber && core && core_strides && u && X && flag, TTR_E_INVALID, "ttr_sample_step: null pointer");
  TTR_REQUIRE(Lnew != L && X != u, TTR_E_INVALID, "ttr_sample_step: Lnew and X must not be inputs");
  const int64_t cs0 = r > 1 ? core_strides[0] : 0, cs1 = I > 1 ? core_strides[1] : 0, cs2 = rn > 1 ? core_strides[2] : 1;
  TTR_REQUIRE(cs2 == 1 && cs0 >= 0 && cs1 >= 0, TTR_E_UNSUPPORTED,
              "ttr_sample_step: the core needs element strides (s0, s1, 1) with s0, s1 >= 0");
  TTR_REQUIRE(ldl >= r && stride_u >= 1 && stride_x >= 1 && (!Lnew || ldn >= rn), TTR_E_UNSUPPORTED,
              "ttr_sample_step: needs ldl >= r, ldn >= r', stride_u >= 1 and stride_x >= 1");
  TTR_REQUIRE(I <= 2147483647LL - 64 && P <= 2147483647LL * 16 &&
                  (double)P * (double)(ldl > ldn ? ldl : ldn) < 9.0e18 / 64.0 &&
                  (double)P * (double)(stride_u > stride_x ? stride_u : stride_x) < 9.0e18 / 64.0 &&
                  (double)r * (double)cs0 + (double)I * (double)cs1 < 9.0e18 / 64.0 && (double)r * (double)I < 9.0e18 / 64.0,
              TTR_E_UNSUPPORTED, "ttr_sample_step: problem too large");
  if (P == 0) return TTR_OK;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return sample_impl<T>({P, r, I, rn, (const T*)L, ldl, (const T*)fiber, (const T*)core, cs0, cs1, cs2, (const double*)u, stride_u,
                           (int64_t*)X, stride_x, (T*)Lnew, ldn, (int*)flag, 0, 0},
                          (hipStream_t)stream);
  });
}
