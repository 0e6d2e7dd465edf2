// The schedule of k_reencode_inter (reencode_kernels.hip) and of k_encode_key / k_encode_inter (encode_kernels.hip), device only: the
// sixteen lanes of a slot as `Lanes` of reencode_mb.hh.  One workgroup's walk over a job's 2:1 wavefront, the body of those kernels, is
// reencode_walk.inc.  See reencode_kernels.hip for why the schedule is what it is.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>

#include "device_types.h"
#include "reencode_mb.hh"

namespace aa {
namespace {

constexpr int kReencSlots = 16;                 // macroblocks of an anti-diagonal in flight: 256 lanes

template <class RegsT>
struct DevLanesOf {
  using Regs = RegsT;
  int b;
  RegsT R;
  template <class F> __device__ __forceinline__ void each( F f ) { f( b, R ); }
  template <class F> __device__ __forceinline__ uint32_t sum( F f )
  {
    uint32_t v = f( b, R );
#pragma unroll
    for ( int m = 8; m >= 1; m >>= 1 ) v += static_cast<uint32_t>( __shfl_xor( static_cast<int>( v ), m, 16 ) );
    return v;
  }
  template <class F> __device__ __forceinline__ int32_t sumi( F f )
  {
    int32_t v = f( b, R );
#pragma unroll
    for ( int m = 8; m >= 1; m >>= 1 ) v += __shfl_xor( v, m, 16 );
    return v;
  }
  // the slot's 16 lanes are one quarter of a wave and run in lock step: what they stored into the slot's LDS picture is ordered for
  // the wave by program order, the compiler is told not to move LDS accesses across
  __device__ __forceinline__ void sync()
  {
    __builtin_amdgcn_fence( __ATOMIC_RELEASE, "wavefront" );
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "wavefront" );
  }
};
using DevLanes = DevLanesOf<ReencRegs>;
using DevLanes2 = DevLanesOf<ReencRegs2>;        // the second pass of a key frame: with the lane's trellis

} // namespace
} // namespace aa
