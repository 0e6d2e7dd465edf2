// The hash chain of the reference -- boost::hash_combine / hash_range (the pre-1.81 formula) over 64-bit size_t -- once, for the host
// and for the device: the step, the description of one chain (a "job") and the walker of a job.
//
// Everything here is marked AA_MHD so that tests/cpp/hash_chain_check.cc can compile the SAME source with g++ and pin it against a
// byte-at-a-time loop of the formula on the CPU; the product only ever walks jobs in device code (k_hash_chains, hash_kernels.hip).
// Reference: BaseRaster::raw_hash (util/raster.cc:52-61), Segmentation::hash (decoder.cc:379-394).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined( __HIPCC__ )
#define AA_MHD __host__ __device__ __forceinline__
#else
#ifndef AA_MHD
#define AA_MHD inline
#endif
#endif

namespace aa {

// One chain: start from seed_in; for each of `rows` rows take row_bytes bytes at src + r * row_stride, then pad_per_row times
// pad_value; then tail_pad times pad_value.  The result is word out_index of the call's result table.
//   a raster      Y, U, V lie back to back in the slot's pool piece: rows = 1, row_bytes = the whole piece
//   a segment map sized by the frame's PIXEL dimensions: mbh rows of mbw map bytes + (width - mbw) threes each, then
//                 (height - mbh) * width threes; seed_in = what the host has combined already (flag, quantiser and filter adjustments)
struct HashJob {
  const uint8_t * src;
  uint64_t seed_in;
  uint64_t row_bytes, row_stride;
  uint64_t tail_pad;
  uint32_t rows, pad_per_row;
  uint32_t out_index, pad_value;
};
static_assert( sizeof( HashJob ) == 56, "the job table is shared by host and device" );

// steps of a job's chain (what the host sorts by, and what the statistics count as bytes walked)
AA_MHD uint64_t hash_job_steps( const HashJob & j ) { return uint64_t( j.rows ) * ( j.row_bytes + j.pad_per_row ) + j.tail_pad; }

// seed ^= v + 0x9e3779b9 + (seed << 6) + (seed >> 2), v a zero-extended byte
AA_MHD uint64_t hash_step( uint64_t seed, uint32_t byte ) { return seed ^ ( uint64_t( byte ) + 0x9e3779b9ull + ( seed << 6 ) + ( seed >> 2 ) ); }
AA_MHD uint64_t hash_word( uint64_t seed, uint32_t w )     // four bytes, lowest address first
{
  seed = hash_step( seed, w & 0xFFu ); seed = hash_step( seed, ( w >> 8 ) & 0xFFu );
  seed = hash_step( seed, ( w >> 16 ) & 0xFFu ); return hash_step( seed, w >> 24 );
}
AA_MHD uint64_t hash_repeat( uint64_t seed, uint32_t value, uint64_t count )
{
  for ( uint64_t i = 0; i < count; i++ ) seed = hash_step( seed, value );
  return seed;
}

struct HashVec16 { uint32_t x, y, z, w; };

// 16 bytes at a 16-byte aligned address: one global_load_dwordx4 on the device
AA_MHD HashVec16 hash_load16( const uint8_t * p )
{
  HashVec16 v;
#if defined( __HIP_DEVICE_COMPILE__ )
  typedef uint32_t u32x4_ __attribute__( ( ext_vector_type( 4 ) ) );
  const u32x4_ q = *reinterpret_cast<const __attribute__( ( address_space( 1 ) ) ) u32x4_ *>( reinterpret_cast<uintptr_t>( p ) );
  v.x = q.x; v.y = q.y; v.z = q.z; v.w = q.w;
#else
  memcpy( &v, p, 16 );
#endif
  return v;
}
AA_MHD uint32_t hash_load8( const uint8_t * p )
{
#if defined( __HIP_DEVICE_COMPILE__ )
  return *reinterpret_cast<const __attribute__( ( address_space( 1 ) ) ) uint8_t *>( reinterpret_cast<uintptr_t>( p ) );
#else
  return *p;
#endif
}

AA_MHD uint64_t hash_vec16( uint64_t seed, const HashVec16 & v )
{
  seed = hash_word( seed, v.x ); seed = hash_word( seed, v.y ); seed = hash_word( seed, v.z ); return hash_word( seed, v.w );
}

// n bytes at p.  Bytes up to the first 16-byte boundary and behind the last one are loaded one by one (a segment map's rows are 3 to
// 120 bytes at any alignment); between them 16 bytes per load through three registers in turn, each refilled as soon as its 16 steps
// are done: the next two loads are in flight under the steps of this one (an HBM miss is about 900 cycles, 16 steps of a lone wave
// about 450).  Nothing outside [p, p + n) is read.
AA_MHD uint64_t hash_bytes( uint64_t seed, const uint8_t * p, uint64_t n )
{
  uint64_t i = 0;
  for ( ; i < n && ( reinterpret_cast<uintptr_t>( p + i ) & 15 ); i++ ) seed = hash_step( seed, hash_load8( p + i ) );
  const uint64_t nvec = ( n - i ) >> 4;
  if ( nvec ) {
    const uint8_t * v = p + i;
    // (a load past the last vector reads the last one again instead: every load is unconditional, so the compiler can count them)
    const uint64_t last = nvec - 1;
    HashVec16 r0 = hash_load16( v ), r1 = hash_load16( v + ( ( 1 < last ? 1 : last ) << 4 ) ), r2 = hash_load16( v + ( ( 2 < last ? 2 : last ) << 4 ) );
    uint64_t k = 0;
    for ( ; k + 3 <= nvec; k += 3 ) {
      seed = hash_vec16( seed, r0 ); r0 = hash_load16( v + ( ( k + 3 < last ? k + 3 : last ) << 4 ) );
      seed = hash_vec16( seed, r1 ); r1 = hash_load16( v + ( ( k + 4 < last ? k + 4 : last ) << 4 ) );
      seed = hash_vec16( seed, r2 ); r2 = hash_load16( v + ( ( k + 5 < last ? k + 5 : last ) << 4 ) );
    }
    if ( k < nvec ) seed = hash_vec16( seed, r0 );
    if ( k + 1 < nvec ) seed = hash_vec16( seed, r1 );
    i += nvec << 4;
  }
  for ( ; i < n; i++ ) seed = hash_step( seed, hash_load8( p + i ) );
  return seed;
}

// The walker of a job: what one lane of k_hash_chains runs, and what the CPU test runs on the host
AA_MHD uint64_t hash_job_walk( const HashJob & j )
{
  uint64_t seed = j.seed_in;
  for ( uint32_t r = 0; r < j.rows; r++ ) {
    seed = hash_bytes( seed, j.src + uint64_t( r ) * j.row_stride, j.row_bytes );
    seed = hash_repeat( seed, j.pad_value, j.pad_per_row );
  }
  return hash_repeat( seed, j.pad_value, j.tail_pad );
}

// The segment-map job of a frame of width x height pixels (mbw x mbh macroblocks) whose map lies at `map`, rows mbw bytes apart;
// seed_in: the chain so far (Segmentation::hash: the absolute flag, then the quantiser and the filter adjustments)
AA_MHD HashJob hash_segment_map_job( const uint8_t * map, uint32_t width, uint32_t height, uint32_t mbw, uint32_t mbh, uint64_t seed_in, uint32_t out_index )
{
  HashJob j;
  j.src = map; j.seed_in = seed_in;
  j.row_bytes = mbw; j.row_stride = mbw;
  j.rows = mbh < height ? mbh : height;                       // (a map has fewer rows than the frame has pixel rows: mbh <= height always)
  j.pad_per_row = width - mbw;
  j.tail_pad = uint64_t( height - j.rows ) * width;
  j.out_index = out_index; j.pad_value = 3;
  return j;
}
AA_MHD HashJob hash_raster_job( const uint8_t * planes, uint64_t bytes, uint32_t out_index )
{
  HashJob j;
  j.src = planes; j.seed_in = 0;
  j.row_bytes = bytes; j.row_stride = bytes;
  j.rows = 1; j.pad_per_row = 0; j.tail_pad = 0;
  j.out_index = out_index; j.pad_value = 0;
  return j;
}

} // namespace aa
