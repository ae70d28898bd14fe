// The centred, weighted sandwich of the ANOVA / Sobol environment recursion on MFMA 16x16x4 (gfx950):
//   ttr_mode_sandwich   Q[s, c, c'] = sum_i w[i] sum_{a, b} (A[a, i, c] - mu[a, c]) Z[s, a, b] (A[b, i, c'] - mu[b, c'])
// One workgroup owns one interface Z[s] and one contiguous chunk of the mode index i.  Z[s] is staged in LDS once, transposed
// ([b][a]: the lanes of an A-operand read run over a); every i of the chunk stages the centred slice A_i - mu [R, C] in LDS (the
// subtraction happens in the registers that carry the global load, mu sits in registers for the whole chunk: a thread stages the
// same (b, c) positions for every i), and wave `v` owns the 16-column strip c' = 16 v .. 16 v + 15 of the output:
//   step 1   Y[:, strip] = Z[s] (A_i - mu)[:, strip]         RT accumulator tiles, they never leave the registers
//   step 2   Q[:, strip] += w[i] (A_i - mu)^T Y[:, strip]    the accumulator tile of step 1 IS the B operand of step 2
// An accumulator tile holds Y[a = row(lane, x)][c' = lane & 15] in register x, and a B operand of k-step x wants
// Y[k][c' = lane & 15] with k chosen by lane >> 4: taking a = 16 t + row(lane, x) as the contraction index of k-step x (for A
// and B alike; a sum does not care about the order of its terms) makes register x the operand as it stands.  Step 1 walks its
// contraction index b in the same order, so both steps read rows {row(lane, x)} of the LDS images: with rows padded by 4 (fp32)
// or 16 (fp64) elements the two row groups of a 32-lane half fall on disjoint banks.
// The chunks' partial sums go to [S, nsplit, C C] in the caller's workspace and ttr_mode_reduce adds them in chunk order (with
// one chunk the kernel writes Q itself): no atomics, workgroups never communicate, and the chunk length follows from (S, I)
// alone, so the same call gives the same bits.  Every global read and write is guarded by its extent; ragged tiles are zeros.
#include "detail/ttr_internal.h"

namespace ttr {

namespace {

constexpr int64_t kSwMaxRank = 64;     // R, C <= 64: four 16-column strips, one per wave
constexpr int64_t kSwMinChunk = 8;     // a workgroup stages Z[s] (R^2) once: at least 8 slices (8 R C) to spend it on
constexpr int64_t kSwTargetBlocks = 512;  // two workgroups per CU
constexpr int64_t kSwMaxS = 65535;     // grid.y

template <typename T>
struct SwArgs {
  int64_t S, R, I, C;
  const T* Z;
  const T* A;
  const T* w;
  const T* mu;
  T* out;  // Q (nsplit == 1) or the partials
  int64_t chunk, nsplit;
};

// slices of i per workgroup: S * nsplit workgroups aim at kSwTargetBlocks, no chunk shorter than kSwMinChunk
int64_t sw_chunk(int64_t S, int64_t I) {
  const int64_t per_s = kSwTargetBlocks / S > 1 ? kSwTargetBlocks / S : 1;
  const int64_t c = ceil_div(I, per_s);
  return c > kSwMinChunk ? c : kSwMinChunk;
}

template <typename T>
constexpr int sw_pad() { return sizeof(T) == 4 ? 4 : 16; }

template <typename T, int RT, int CT>
constexpr size_t sw_lds_bytes() {
  return sizeof(T) * (size_t)(RT * 16) * (size_t)((RT * 16 + sw_pad<T>()) + (CT * 16 + sw_pad<T>()));
}

template <typename T, int RT, int CT>
__global__ __launch_bounds__(kThreads) void sandwich_kernel(SwArgs<T> p) {
  constexpr int RP = RT * 16, CP = CT * 16;
  constexpr int LDZ = RP + sw_pad<T>(), LDA = CP + sw_pad<T>();
  constexpr int EA = RT * CT;  // RP * CP / kThreads staged elements of a slice per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char sw_smem[];
  T* Zt = (T*)sw_smem;      // [b][a], RP x LDZ
  T* As = Zt + RP * LDZ;    // [b][c], RP x LDA
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l15 = lane & 15;
  const int64_t s = blockIdx.y;
  const int64_t k = blockIdx.x;
  const int64_t i0 = k * p.chunk;
  const int64_t i1 = i0 + p.chunk < p.I ? i0 + p.chunk : p.I;
  const int R = (int)p.R, C = (int)p.C;

  {  // Z[s] -> LDS, transposed; rows / columns past R are zeros
    const T* __restrict__ Zs = p.Z + s * p.R * p.R;
    for (int idx = tid; idx < RP * RP; idx += kThreads) {
      const int a = idx / RP, b = idx % RP;
      Zt[b * LDZ + a] = (a < R && b < R) ? Zs[(int64_t)a * R + b] : T(0);
    }
  }

  // the (b, c) this thread stages of every slice, and mu there
  int64_t aoff[EA];
  int loff[EA];
  bool ok[EA];
  T m[EA], ra[EA];
#pragma unroll
  for (int e = 0; e < EA; ++e) {
    const int idx = tid + kThreads * e;
    const int b = idx / CP, c = idx % CP;
    ok[e] = b < R && c < C;
    aoff[e] = (int64_t)b * p.I * p.C + c;
    loff[e] = b * LDA + c;
    m[e] = (ok[e] && p.mu) ? p.mu[(int64_t)b * C + c] : T(0);
  }
  auto fetch = [&](int64_t i) {
#pragma unroll
    for (int e = 0; e < EA; ++e) ra[e] = ok[e] ? p.A[aoff[e] + i * p.C] - m[e] : T(0);
  };

  typename Mfma<T>::Acc q[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) q[t] = Mfma<T>::zero();

  fetch(i0);
  for (int64_t i = i0; i < i1; ++i) {
#pragma unroll
    for (int e = 0; e < EA; ++e) As[loff[e]] = ra[e];
    const T wi = p.w ? p.w[i] : T(1);
    __syncthreads();
    if (i + 1 < i1) fetch(i + 1);  // in flight under the MFMAs below
    if (wave < CT) {
      typename Mfma<T>::Acc y[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t) y[t] = Mfma<T>::zero();
#pragma unroll
      for (int bt = 0; bt < RT; ++bt)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int brow = bt * 16 + Mfma<T>::row(lane, x);
          const T bf = As[brow * LDA + wave * 16 + l15];
#pragma unroll
          for (int t = 0; t < RT; ++t) y[t] = Mfma<T>::mma(Zt[brow * LDZ + t * 16 + l15], bf, y[t]);
        }
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int arow = t * 16 + Mfma<T>::row(lane, x);
          const T yv = y[t][x] * wi;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) q[ct] = Mfma<T>::mma(As[arow * LDA + ct * 16 + l15], yv, q[ct]);
        }
    }
    __syncthreads();
  }

  if (wave < CT) {
    T* __restrict__ out = p.out + (s * p.nsplit + k) * p.C * p.C;
    const int col = wave * 16 + l15;
    if (col < C) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int row = ct * 16 + Mfma<T>::row(lane, x);
          if (row < C) out[(int64_t)row * C + col] = q[ct][x];
        }
    }
  }
}

template <typename T, int RT, int CT>
int sandwich_launch_rc(const SwArgs<T>& p, hipStream_t stream) {
  constexpr size_t lds = sw_lds_bytes<T, RT, CT>();
  auto kern = sandwich_kernel<T, RT, CT>;
  if (lds > 64 * 1024) TTR_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)p.nsplit, (unsigned)p.S), dim3(kThreads), lds, stream, p);
  return TTR_OK;
}

template <typename T, int RT>
int sandwich_launch_r(const SwArgs<T>& p, int ct, hipStream_t stream) {
  switch (ct) {
    case 1: return sandwich_launch_rc<T, RT, 1>(p, stream);
    case 2: return sandwich_launch_rc<T, RT, 2>(p, stream);
    case 3: return sandwich_launch_rc<T, RT, 3>(p, stream);
    default: return sandwich_launch_rc<T, RT, 4>(p, stream);
  }
}

template <typename T>
int sandwich_impl(SwArgs<T> p, void* Q, void* ws, hipStream_t stream) {
  p.out = p.nsplit > 1 ? (T*)ws : (T*)Q;
  const int rt = (int)ceil_div(p.R, 16), ct = (int)ceil_div(p.C, 16);
  {
    ProfScope prof(TTR_PROF_MISC, stream);
    int rc;
    switch (rt) {
      case 1: rc = sandwich_launch_r<T, 1>(p, ct, stream); break;
      case 2: rc = sandwich_launch_r<T, 2>(p, ct, stream); break;
      case 3: rc = sandwich_launch_r<T, 3>(p, ct, stream); break;
      default: rc = sandwich_launch_r<T, 4>(p, ct, stream); break;
    }
    if (rc != TTR_OK) return rc;
    TTR_HIP_CHECK(hipGetLastError());
  }
  if (p.nsplit == 1) return TTR_OK;
  // Q[s, :] = sum_k partial[s, k, :], k increasing
  const int64_t cc = p.C * p.C;
  const int64_t xs[3] = {p.nsplit * cc, cc, 1}, ys[2] = {cc, 1};
  return ttr_mode_reduce(sizeof(T) == 4 ? TTR_F32 : TTR_F64, p.S, p.nsplit, cc, ws, xs, nullptr, 1.0, Q, ys, (void*)stream);
}

int sandwich_check(int dtype, int64_t S, int64_t R, int64_t I, int64_t C) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_mode_sandwich: bad dtype %d", dtype);
  TTR_REQUIRE(S >= 1 && R >= 1 && I >= 1 && C >= 1, TTR_E_INVALID, "ttr_mode_sandwich: bad sizes S = %lld, R = %lld, I = %lld, C = %lld",
              (long long)S, (long long)R, (long long)I, (long long)C);
  TTR_REQUIRE(R <= kSwMaxRank && C <= kSwMaxRank, TTR_E_UNSUPPORTED, "ttr_mode_sandwich: ranks %lld x %lld above %lld", (long long)R,
              (long long)C, (long long)kSwMaxRank);
  TTR_REQUIRE(S <= kSwMaxS, TTR_E_UNSUPPORTED, "ttr_mode_sandwich: S = %lld > %lld", (long long)S, (long long)kSwMaxS);
  TTR_REQUIRE(I <= (int64_t)(9.0e18 / 64.0) / (kSwMaxRank * kSwMaxRank), TTR_E_UNSUPPORTED, "ttr_mode_sandwich: core too large");
  return TTR_OK;
}

}  // namespace

}  // namespace ttr

using namespace ttr;

extern "C" int ttr_mode_sandwich_max_rank(void) { return (int)kSwMaxRank; }

extern "C" int64_t ttr_mode_sandwich_workspace_bytes(int dtype, int64_t S, int64_t R, int64_t I, int64_t C) {
  const int rc = sandwich_check(dtype, S, R, I, C);
  if (rc != TTR_OK) return rc;
  const int64_t nsplit = ceil_div(I, sw_chunk(S, I));
  return nsplit > 1 ? align_up(S * nsplit * C * C * elem_size(dtype), 256) : 0;
}

extern "C" int ttr_mode_sandwich(int dtype, int64_t S, int64_t R, int64_t I, int64_t C, const void* Z, const void* A,
                                 const int64_t* a_strides, const void* w, const void* mu, void* Q, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  const int64_t need = ttr_mode_sandwich_workspace_bytes(dtype, S, R, I, C);
  if (need < 0) return (int)need;
  TTR_REQUIRE(Z && A && Q && a_strides, TTR_E_INVALID, "ttr_mode_sandwich: null pointer");
  TTR_REQUIRE(Q != Z && Q != A && Q != w && Q != mu, TTR_E_INVALID, "ttr_mode_sandwich: Q must not alias an input");
  const int64_t as[3] = {R, I, C};
  TTR_REQUIRE(contiguous(as, a_strides, 3), TTR_E_UNSUPPORTED, "ttr_mode_sandwich: A must be contiguous");
  TTR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), TTR_E_WORKSPACE, "ttr_mode_sandwich: workspace %lld < %lld bytes",
              (long long)workspace_bytes, (long long)need);
  const int64_t chunk = sw_chunk(S, I);
  const int64_t nsplit = ceil_div(I, chunk);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return sandwich_impl<T>({S, R, I, C, (const T*)Z, (const T*)A, (const T*)w, (const T*)mu, nullptr, chunk, nsplit}, Q, workspace,
                            (hipStream_t)stream);
  });
}
