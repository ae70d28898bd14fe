// The backward of the differentiable point evaluation t[X] (tntorch_amd/autodiff.py): the gradient of one core from the samples.
//
// With the left interfaces L [P, r0] and the right interfaces R [P, r1] of a mode (R seeded with the incoming gradient),
//   dG[:, i, :] = sum over the samples p of slice i of  L[p]^T R[p]
// a segmented GEMM whose K dimension is the sample axis.  Torch ops materialise the P x r0 x r1 outer products before an
// index_add_; here
//   gather_grad_kernel   one workgroup per (task, 64 x 64 tile of (a, b)): the task's rows of L and R (the tile's columns only)
//                        are gathered through `perm` into LDS S samples at a time, and every wave accumulates a 16 x 64 strip on
//                        the matrix cores (16x16x4, four samples per instruction).  The one task of a slice writes dG directly, a
//                        task of a slice with several writes its partial tile to the workspace;
//   gather_grad_reduce   sums the partials of a slice with several tasks in task order and zeroes the slices with none.
// No atomics: the same inputs give the same bits.
#include "detail/ttr_internal.h"

namespace ttr {
namespace {

constexpr int kTile = 64;                   // (a, b) tile of one workgroup: wave w owns rows [16 w, 16 w + 16), four 16-column tiles
constexpr int64_t kStageBytes = 48 * 1024;  // LDS of the staged rows
constexpr int64_t kMaxRank = 512;           // ttr_gather_step's limit

// staged row width (elements) of a tile side of `r` columns: the live columns rounded up to 16, and 16 more where that is a
// multiple of 32, so that the row stride is 16 mod 32: the four sample rows an MFMA operand reads (16 lanes each) fall on
// different banks, in fp32 (ds_read_b32, 2 x 32 lanes) and in fp64 (ds_read_b64)
inline int64_t stage_width(int64_t r) { return (std::min<int64_t>(kTile, align_up(r, 16))) | 16; }

int64_t stage_rows(int dtype, int64_t r0, int64_t r1) {  // samples per pass: a multiple of 4, <= 256
  const int64_t S = kStageBytes / ((stage_width(r0) + stage_width(r1)) * elem_size(dtype) + 8);
  return (S > 256 ? 256 : S) & ~(int64_t)3;
}

// grid (ntasks, tiles of a x tiles of b).  LDS: sL [S][la], sR [S][lb], sQ [S]
template <typename T>
__global__ void __launch_bounds__(kThreads) gather_grad_kernel(int64_t I, int r0, int r1, int S, int la, int lb,
                                                                const T* __restrict__ L, int64_t ldl, const T* __restrict__ R,
                                                                int64_t ldr, const int64_t* __restrict__ perm,
                                                                const int64_t* __restrict__ tb, const int64_t* __restrict__ te,
                                                                const int64_t* __restrict__ toff, T* __restrict__ dG,
                                                                T* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ int64_t s_slice;
  T* sL = (T*)smem_raw;
  T* sR = sL + (int64_t)S * la;
  int64_t* sQ = (int64_t*)(sR + (int64_t)S * lb);
  using M = Mfma<T>;
  const int64_t task = blockIdx.x;
  const int ntb = (r1 + kTile - 1) / kTile;
  const int a0 = ((int)blockIdx.y / ntb) * kTile, b0 = ((int)blockIdx.y % ntb) * kTile;
  const int wa = min(kTile, r0 - a0), wb = min(kTile, r1 - b0);  // live columns of the tile's two sides
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  if (tid == 0) {  // slice of this task: the largest i with toff[i] <= task
    int64_t lo = 0, hi = I - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (toff[mid] <= task) lo = mid; else hi = mid - 1;
    }
    s_slice = lo;
  }
  const int64_t b = tb[task], e = te[task];
  const bool wave_live = wave * 16 < wa;
  typename M::Acc acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = M::zero();

  for (int64_t c0 = b; c0 < e; c0 += S) {
    const int n = (int)min((int64_t)S, e - c0);
    const int n4 = (n + 3) & ~3;  // rows n .. n4 - 1 are staged as zeros: S is a multiple of 4, so n4 <= S
    __syncthreads();
    for (int p = tid; p < n4; p += kThreads) sQ[p] = p < n ? perm[c0 + p] : -1;
    __syncthreads();
    for (int x = tid; x < n4 * la; x += kThreads) {
      const int p = x / la, a = x - p * la;
      const int64_t q = sQ[p];
      sL[x] = (q >= 0 && a < wa) ? L[q * ldl + a0 + a] : T(0);
    }
    for (int x = tid; x < n4 * lb; x += kThreads) {
      const int p = x / lb, c = x - p * lb;
      const int64_t q = sQ[p];
      sR[x] = (q >= 0 && c < wb) ? R[q * ldr + b0 + c] : T(0);
    }
    __syncthreads();
    if (wave_live) {
      const T* pa = sL + (lane >> 4) * la + wave * 16 + (lane & 15);  // A[i = a][k = sample]
      const T* pb = sR + (lane >> 4) * lb + (lane & 15);              // B[k = sample][j = b]
      for (int k0 = 0; k0 < n4; k0 += 4) {
        const T av = pa[k0 * la];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (u * 16 < wb) acc[u] = M::mma(av, pb[k0 * lb + u * 16], acc[u]);  // (wave-uniform; columns < lb: lb >= 16 ceil(wb / 16))
      }
    }
  }
  __syncthreads();  // s_slice (an empty task never reached a barrier)
  const int64_t i = s_slice;
  const bool direct = toff[i + 1] - toff[i] == 1;
  // dG [r0, I, r1]; a partial is a compact [r0, r1] matrix
  T* out = direct ? dG + i * r1 : part + task * (int64_t)r0 * r1;
  const int64_t ld = direct ? I * (int64_t)r1 : (int64_t)r1;
  if (!wave_live) return;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = u * 16 + (lane & 15);
    if (c >= wb) continue;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int a = wave * 16 + M::row(lane, reg);
      if (a < wa) out[(a0 + a) * ld + b0 + c] = acc[u][reg];
    }
  }
}

// grid (I, chunks of r0 r1): a slice with one task was written by its task; none: zeros; several: their sum in task order
template <typename T>
__global__ void __launch_bounds__(kThreads) gather_grad_reduce(int64_t I, int r0, int r1, const int64_t* __restrict__ toff,
                                                                const T* __restrict__ part, T* __restrict__ dG) {
  const int64_t i = blockIdx.x;
  const int64_t t0 = toff[i], t1 = toff[i + 1];
  if (t1 - t0 == 1) return;
  const int64_t K = (int64_t)r0 * r1;
  const int64_t x = (int64_t)blockIdx.y * kThreads + threadIdx.x;
  if (x >= K) return;
  T s = T(0);
  for (int64_t t = t0; t < t1; ++t) s += part[t * K + x];
  const int64_t a = x / r1, c = x - a * r1;
  dG[(a * I + i) * r1 + c] = s;
}

}  // namespace
}  // namespace ttr

using namespace ttr;

extern "C" int64_t ttr_gather_grad_stage_rows(int dtype, int64_t r0, int64_t r1) {
  if (!dtype_ok(dtype) || r0 < 1 || r1 < 1 || r0 > kMaxRank || r1 > kMaxRank) return -1;
  return stage_rows(dtype, r0, r1);
}

extern "C" int64_t ttr_gather_grad_workspace_bytes(int dtype, int64_t ntasks, int64_t r0, int64_t r1) {
  if (!dtype_ok(dtype) || ntasks < 0 || r0 < 1 || r1 < 1) return -1;
  return ntasks * r0 * r1 * elem_size(dtype);
}

extern "C" int ttr_gather_grad(int dtype, int64_t I, int64_t ntasks, int64_t r0, int64_t r1, const void* L, int64_t ldl,
                               const void* R, int64_t ldr, const void* perm, const void* task_begin, const void* task_end,
                               const void* task_off, void* dG, void* workspace, int64_t workspace_bytes, void* stream) {
  TTR_REQUIRE(dtype_ok(dtype), TTR_E_INVALID, "ttr_gather_grad: bad dtype %d", dtype);
  TTR_REQUIRE(I >= 1 && ntasks >= 0 && r0 >= 1 && r1 >= 1 && ldl >= r0 && ldr >= r1, TTR_E_INVALID, "ttr_gather_grad: bad sizes");
  TTR_REQUIRE(r0 <= kMaxRank && r1 <= kMaxRank, TTR_E_UNSUPPORTED, "ttr_gather_grad: rank above %lld", (long long)kMaxRank);
  TTR_REQUIRE(ntasks < ((int64_t)1 << 31) && I < ((int64_t)1 << 31), TTR_E_UNSUPPORTED, "ttr_gather_grad: too many tasks or slices");
  TTR_REQUIRE(dG, TTR_E_INVALID, "ttr_gather_grad: NULL output");
  const int64_t es = elem_size(dtype);
  hipStream_t s = (hipStream_t)stream;
  if (ntasks == 0) {
    TTR_HIP_CHECK(hipMemsetAsync(dG, 0, (size_t)(r0 * I * r1 * es), s));
    return TTR_OK;
  }
  TTR_REQUIRE(L && R && perm && task_begin && task_end && task_off, TTR_E_INVALID, "ttr_gather_grad: NULL argument");
  const int64_t need = ntasks * r0 * r1 * es;
  TTR_REQUIRE(workspace && workspace_bytes >= need, TTR_E_WORKSPACE, "ttr_gather_grad: workspace %lld < %lld bytes",
              (long long)workspace_bytes, (long long)need);
  const int64_t S = stage_rows(dtype, r0, r1), la = stage_width(r0), lb = stage_width(r1);
  const size_t lds = (size_t)(S * (la + lb) * es + S * 8);
  const dim3 grid((unsigned)ntasks, (unsigned)(ceil_div(r0, kTile) * ceil_div(r1, kTile)));
  const dim3 rgrid((unsigned)I, (unsigned)ceil_div(r0 * r1, kThreads));
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(gather_grad_kernel<T>, grid, dim3(kThreads), lds, s, I, (int)r0, (int)r1, (int)S, (int)la, (int)lb,
                       (const T*)L, ldl, (const T*)R, ldr, (const int64_t*)perm, (const int64_t*)task_begin,
                       (const int64_t*)task_end, (const int64_t*)task_off, (T*)dG, (T*)workspace);
    hipLaunchKernelGGL(gather_grad_reduce<T>, rgrid, dim3(kThreads), 0, s, I, (int)r0, (int)r1, (const int64_t*)task_off,
                       (const T*)workspace, (T*)dG);
  });
  TTR_HIP_CHECK(hipGetLastError());
  return TTR_OK;
}
