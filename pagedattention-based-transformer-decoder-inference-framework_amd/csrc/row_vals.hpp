// A vocabulary row held by one workgroup in registers + LDS, and the block
// reduction over it: shared by the row kernels of csrc/sample.hip (token
// sampling) and csrc/beam_select.hip (beam candidates).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace llm {

constexpr int kSampleThreads = 512;  // 8 waves: 256 VGPRs per lane available

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* sh, Op op) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = sh[0];
  for (int i = 1; i < kSampleThreads / 64; ++i) t = op(t, sh[i]);  // fixed order
  return t;
}

// Thread t owns the contiguous tokens [t*VPT, t*VPT + VPT) of the row.  The
// first VPT_REG of them live in registers, the rest in LDS (VPT 128: 128 KiB,
// [slot][thread] so each access is bank-conflict free).
template <int VPT>
struct RowVals {
  // register slots; the rest in LDS: VPT 64 -> 32 + 64 KiB, VPT 128 -> 56 + 144 KiB
  static constexpr int R = VPT <= 32 ? VPT : (VPT <= 64 ? 32 : 56);
  float reg[R];
  // volatile: re-read per use, so the compiler does not hoist the LDS half into
  // registers across the radix-search loops (that spilled)
  volatile float* lds;  // [(VPT - R)][kSampleThreads]
  // f(i, value&): register slots unrolled, LDS slots in a rolled loop (dynamic
  // LDS indexing is free; unrolling it only made the compiler hoist and spill)
  template <typename F>
  __device__ __forceinline__ void each(F f) {
#pragma unroll
    for (int i = 0; i < R; ++i) f(i, reg[i]);
#pragma unroll 1
    for (int i = R; i < VPT; ++i) {
      float v = lds[(i - R) * kSampleThreads + threadIdx.x];
      f(i, v);
      lds[(i - R) * kSampleThreads + threadIdx.x] = v;
    }
  }
};

}  // namespace llm
