// DCT partitions of VP8 frames written on the device from the records (aa_serialize_batch): Frame::serialize_tokens
// (serializer.cc:407-443, 595-739) for many frames at once.
//
//   k_serialize_tokens   lane l < lanes_per_wave of workgroup g (one wave) takes entry g * lanes_per_wave + l of the call's lane list: one
//                        (job, DCT partition).  It walks the macroblock rows row % partitions == partition of the job's frame in raster
//                        order -- records and coefficients where reconstruction reads them, dense or packed -- and writes their tokens with
//                        the boolean encoder of bool_writer.hh into its own range of the call's staging piece: plain byte stores, a carry
//                        re-reads and rewrites bytes the same lane stored.  A bool is a chain of dependent integer instructions and a
//                        block's contexts come from the neighbours' records (serialize_common.hh), so there is nothing to share between
//                        lanes: no LDS, no atomics, no waiting.  Every loop is bounded by the frame's macroblock count (the Y2 walk
//                        by its rows).  As with the hash chains (hash_kernels.hip) the kernel is bound by a wave's instruction issue and
//                        the lanes of a wave take different branches, so the host spreads the lanes over the chip's SIMDs before any
//                        wave gets a second one.
//                        A byte that has no room in the lane's range is counted, not stored; sizes[partition] is what the partition
//                        takes either way, and the host refuses a frame whose partitions did not fit.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "serialize_common.hh"

namespace aa {
namespace {

__global__ __launch_bounds__( 64 ) void k_serialize_tokens( const aa_serialize_dev_job * jobs, const uint32_t * lanes, uint32_t n_lanes, uint32_t lanes_per_wave )
{
  if ( threadIdx.x >= lanes_per_wave ) return;
  const uint32_t i = blockIdx.x * lanes_per_wave + threadIdx.x;
  if ( i >= n_lanes ) return;
  const uint32_t entry = lanes[i];
  const aa_serialize_dev_job & J = jobs[entry >> 3];
  const uint32_t part = entry & 7u;
  if ( part >= J.nparts ) return;
  const aa_dev_frame & f = *J.frame;
  BoolWriter w( J.out + static_cast<size_t>( part ) * J.region, J.region );
  J.sizes[part] = ser::write_partition( w, J.probs, f.mbs, f.mbw, f.mbh, f.coeffs, f.packed != 0, J.skip_enabled != 0, part, J.nparts );
}

// The reference's probability passes in front of the token kernel, for the jobs that ask for them (optimise):
//
//   k_token_counts   workgroup (x, job) takes macroblocks [x * run, (x + 1) * run) of the job's frame, sixteen at a time, 16 lanes each: lane b
//                    walks luma block b, lanes 0..7 then the chroma blocks 16 + b, as accumulate_token_branches does (Y2 blocks are NOT
//                    counted: serializer.cc:582-586; a Y block beside a Y2 block starts at position 1; EVERY macroblock is counted, also the
//                    ones whose tokens are skipped: reencode.cc:116,292 count before mb_skip_coeff is decided).  A block's context comes from
//                    the nz_mask of the macroblock and its neighbours' records, so nothing is serial.  Counts [4][8][3][11][2] in LDS with LDS
//                    atomics, added to the job's table in HBM with vector atomics once per workgroup; the same launch counts, by __ballot over
//                    the records, the macroblocks that have coefficients and the macroblocks of each reference frame.
//   k_token_probs    one thread per (job, probability): calc_prob of its two counts, the update decision against the table before the frame
//                    (prob > 0 && prob != current), the frame's table in place and the update flags / values for the host's header; four
//                    more threads make prob_skip_false and the three reference probabilities.
constexpr uint32_t kCountRun = 64;      // macroblocks per workgroup of k_token_counts

__global__ __launch_bounds__( 256 ) void k_token_counts( const aa_serialize_dev_job * jobs )
{
  __shared__ uint32_t cnt[AA_SERIALIZE_COUNTS];
  const aa_serialize_dev_job & J = jobs[blockIdx.y];
  if ( !J.optimise ) return;                                         // (the whole workgroup)
  const aa_dev_frame & f = *J.frame;
  const uint32_t mbw = f.mbw, nmb = static_cast<uint32_t>( f.mbw ) * f.mbh;
  const uint32_t begin = blockIdx.x * kCountRun, end = begin + kCountRun < nmb ? begin + kCountRun : nmb;
  if ( begin >= nmb ) return;                                        // (the whole workgroup)
  for ( uint32_t i = threadIdx.x; i < AA_SERIALIZE_COUNTS; i += 256 ) cnt[i] = 0;
  __syncthreads();
  const uint32_t b16 = threadIdx.x & 15u, slot = threadIdx.x >> 4;
  const bool packed = f.packed != 0;
  for ( uint32_t m0 = begin; m0 < end; m0 += 16 ) {
    const uint32_t mi = m0 + slot;
    const bool valid = mi < end;
    uint32_t nz = 0, ref = 0;
    if ( valid ) {
      const aa_mb_info & mb = f.mbs[mi];
      const uint32_t col = mi % mbw, row = mi / mbw;
      nz = ser::context_mask( mb ); ref = mb.ref_frame & 3u;
      const uint32_t above = row ? ser::context_mask( f.mbs[mi - mbw] ) : 0u, left = col ? ser::context_mask( f.mbs[mi - 1] ) : 0u;
      const bool has_y2 = mb.flags & AA_MB_HAS_Y2;
      const int16_t * const base = packed ? f.coeffs + ( static_cast<size_t>( mb.reserved ) << 32 | mb.coeff_index ) : f.coeffs + static_cast<size_t>( mb.coeff_index ) * 16;
      for ( uint32_t b = b16; b < 24; b += 16 ) {                      // luma b16, then (lanes 0..7) chroma 16 + b16
        uint32_t zmask = 0;
        const int16_t * v = base;
        if ( ( nz >> b ) & 1u ) {
          if ( packed ) {
            uint32_t off = 25u + ( ( nz >> 24 ) & 1u ? ser::popc( static_cast<uint16_t>( base[24] ) ) : 0u );
            for ( uint32_t p = 0; p < b; p++ ) if ( ( nz >> p ) & 1u ) off += ser::popc( static_cast<uint16_t>( base[p] ) );
            v = base + off; zmask = static_cast<uint16_t>( base[b] );
          } else {
            v = base + 16u * ( ( ( nz >> 24 ) & 1u ) + ser::popc( nz & ( ( 1u << b ) - 1u ) ) );
            for ( uint32_t j = 0; j < 16; j++ ) if ( v[j] ) zmask |= 1u << ( static_cast<uint32_t>( ser::kInvZigzagNib >> ( 4 * j ) ) & 15u );
          }
        }
        const uint32_t type = b >= 16 ? 2u : ( has_y2 ? 0u : 3u ), first = ( b < 16 && has_y2 ) ? 1u : 0u;
        ser::count_block( [&]( const uint32_t node, const uint32_t taken ) { atomicAdd( &cnt[2u * node + taken], 1u ); }, type, first,
                          ser::block_context( b, nz, above, left ), zmask,
                          [=]( const uint32_t k ) { return static_cast<int>( packed ? v[ser::popc( zmask & ( ( 1u << k ) - 1u ) )] : v[ser::zigzag( k )] ); } );
      }
    }
    // the macroblocks' own classes: one lane per macroblock votes, one lane per wave adds
    const bool head = valid && b16 == 0;
    const unsigned long long has = __ballot( head && nz != 0 );
    const unsigned long long r0 = __ballot( head && ref == 0 ), r1 = __ballot( head && ref == 1 ), r2 = __ballot( head && ref == 2 ), r3 = __ballot( head && ref == 3 );
    if ( ( threadIdx.x & 63u ) == 0 ) {
      atomicAdd( &cnt[2112], static_cast<uint32_t>( __popcll( has ) ) );
      atomicAdd( &cnt[2113], static_cast<uint32_t>( __popcll( r0 ) ) ); atomicAdd( &cnt[2114], static_cast<uint32_t>( __popcll( r1 ) ) );
      atomicAdd( &cnt[2115], static_cast<uint32_t>( __popcll( r2 ) ) ); atomicAdd( &cnt[2116], static_cast<uint32_t>( __popcll( r3 ) ) );
    }
  }
  __syncthreads();
  for ( uint32_t i = threadIdx.x; i < AA_SERIALIZE_COUNTS; i += 256 ) if ( cnt[i] ) atomicAdd( &J.counts[i], cnt[i] );
}

__global__ __launch_bounds__( 256 ) void k_token_probs( aa_serialize_dev_job * jobs )
{
  aa_serialize_dev_job & J = jobs[blockIdx.y];
  if ( !J.optimise ) return;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t * c = J.counts;
  if ( i < 1056 ) {
    uint32_t prob = ser::calc_prob( c[2 * i], c[2 * i] + c[2 * i + 1] );
    bool update = prob > 0 && prob != J.probs[i];
    if ( !update && J.first_pass && J.first_pass[i] ) { update = true; prob = J.first_pass[1056 + i]; }      // (a two-pass key frame: the first pass's update stands)
    J.updates[i] = update; J.updates[1056 + i] = update ? static_cast<uint8_t>( prob ) : 0;
    if ( update ) J.probs[i] = static_cast<uint8_t>( prob );
  } else if ( i == 1056 ) J.updates[2112] = static_cast<uint8_t>( ser::calc_prob( c[2112], static_cast<uint32_t>( J.frame->mbw ) * J.frame->mbh ) );   // optimize_prob_skip
  else if ( i == 1057 ) J.updates[2113] = static_cast<uint8_t>( ser::calc_prob( c[2113], c[2113] + c[2114] + c[2115] + c[2116] ) );                     // optimize_interframe_probs
  else if ( i == 1058 ) J.updates[2114] = static_cast<uint8_t>( ser::calc_prob( c[2114], c[2114] + c[2115] + c[2116] ) );
  else if ( i == 1059 ) J.updates[2115] = static_cast<uint8_t>( ser::calc_prob( c[2115], c[2115] + c[2116] ) );
}

} // namespace

int launch_serialize_probs( aa_serialize_dev_job * jobs, int n, uint32_t max_mbs, void * stream )
{
  if ( n <= 0 || !max_mbs ) return static_cast<int>( hipErrorInvalidValue );
  hipLaunchKernelGGL( k_token_counts, dim3( ( max_mbs + kCountRun - 1 ) / kCountRun, n ), dim3( 256 ), 0, static_cast<hipStream_t>( stream ), jobs );
  if ( hipError_t e = hipGetLastError() ) return static_cast<int>( e );
  hipLaunchKernelGGL( k_token_probs, dim3( 5, n ), dim3( 256 ), 0, static_cast<hipStream_t>( stream ), jobs );
  return static_cast<int>( hipGetLastError() );
}

int launch_serialize_tokens( const aa_serialize_dev_job * jobs, const uint32_t * lanes, int n_lanes, int lanes_per_wave, void * stream )
{
  if ( n_lanes <= 0 || lanes_per_wave < 1 || lanes_per_wave > 64 ) return static_cast<int>( hipErrorInvalidValue );
  const unsigned waves = ( static_cast<unsigned>( n_lanes ) + lanes_per_wave - 1 ) / lanes_per_wave;
  hipLaunchKernelGGL( k_serialize_tokens, dim3( waves ), dim3( 64 ), 0, static_cast<hipStream_t>( stream ), jobs, lanes, static_cast<uint32_t>( n_lanes ),
                      static_cast<uint32_t>( lanes_per_wave ) );
  return static_cast<int>( hipGetLastError() );
}

} // namespace aa
