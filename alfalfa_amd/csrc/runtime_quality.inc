// runtime.cpp (ABI), between the rasters and the loop-filter search: planes scored against originals on the device -- decoded frames
// (aa_quality_batch_async) and the candidates of the loop-filter search (runtime_lf_search.inc); kernels in quality_kernels.hip.
extern "C" {
namespace {
struct QualityPair { const uint8_t * a; int64_t stride_a; const uint8_t * b; int64_t stride_b; uint32_t w, h; };   // device planes, w x h pixels

// SSIM (and, with sse_dev, the squared error) of np pairs of planes in device memory: one k_quality_blocks launch over all of them
// and one k_quality_sum, on the compute stream.  The job table goes through a ring of pinned buffers into the call's piece of the
// device pool, which also holds the group values; the piece goes back by the compute-stream route.  Nothing comes to the host.
aa_status quality_of_planes( aa_ctx * ctx, const QualityPair * pairs, int np, double * ssim_dev, uint64_t * sse_dev, hipStream_t consumer )
{
  const size_t table_bytes = align_up( size_t( np ) * sizeof( aa_quality_job ) );
  JobRing::Entry * qb = nullptr;
  if ( aa_status st = ctx->quality_ring.take( table_bytes, align_up( 1536 * sizeof( aa_quality_job ) ), &qb ) ) return st;
  aa_quality_job * jobs = reinterpret_cast<aa_quality_job *>( qb->host );
  uint64_t floats = 0;
  uint32_t max_blocks = 0;
  for ( int i = 0; i < np; i++ ) {
    const QualityPair & p = pairs[i];
    aa_quality_job & j = jobs[i];
    j.a = p.a; j.stride_a = p.stride_a;
    j.b = p.b; j.stride_b = p.stride_b;
    j.w4 = p.w >> 2; j.h4 = p.h >> 2;
    j.groups = ( j.w4 - 1 + 3 ) / 4;
    j.strips = ( j.h4 - 1 + AA_QUALITY_STRIP_ROWS - 1 ) / AA_QUALITY_STRIP_ROWS;
    j.chunks = ( j.w4 - 1 + AA_QUALITY_CHUNK_WINDOWS - 1 ) / AA_QUALITY_CHUNK_WINDOWS;
    j.pad = 0;
    j.out_off = floats;
    floats += ( uint64_t( j.h4 - 1 ) * j.groups + 3 ) & ~uint64_t( 3 );
    max_blocks = std::max( max_blocks, j.strips * j.chunks );
  }
  const size_t piece_bytes = table_bytes + floats * sizeof( float );
  uint8_t * piece = nullptr;
  if ( aa_status st = dev_alloc_compute( ctx, piece_bytes, &piece ) ) return st;
  // (only the compute stream touches the piece: the next owner's kernels are behind this call's)
  struct Back { aa_ctx * c; uint8_t * p; size_t b; ~Back() { dev_free_compute( c, p, b ); } } back { ctx, piece, piece_bytes };
  if ( aa_status st = stream_waits_for( &ctx->quality_consumer_ev, ctx->compute, consumer ) ) return st;
  HIP_TRY( hipMemcpyAsync( piece, qb->host, size_t( np ) * sizeof( aa_quality_job ), hipMemcpyHostToDevice, ctx->compute ) );
  if ( aa_status st = ctx->quality_ring.mark( *qb, ctx->compute ) ) return st;
  if ( sse_dev ) HIP_TRY( hipMemsetAsync( sse_dev, 0, size_t( np ) * sizeof( uint64_t ), ctx->compute ) );
  if ( int e = aa::launch_quality( reinterpret_cast<const aa_quality_job *>( piece ), np, max_blocks, reinterpret_cast<float *>( piece + table_bytes ),
                                   ssim_dev, reinterpret_cast<unsigned long long *>( sse_dev ), ctx->compute ) )
    return hip_fail( static_cast<hipError_t>( e ), "k_quality_blocks / k_quality_sum" );
  return stream_waits_for( &ctx->quality_consumer_ev, consumer, ctx->compute );
}
} // namespace

/* BaseRaster::quality (util/raster.cc:63-66) and the squared error of n decoded frames against n originals in device memory, on the
 * compute stream behind the decode of those frames -- rasters are recycled in compute-stream order, so a frame released right after
 * the call is still read intact.  (quality_of_planes does the work.) */
aa_status aa_quality_batch_async( aa_ctx * ctx, aa_stream * const * streams, int n, const int * frame_index, const aa_quality_ref * originals,
                                  int planes, double * ssim_dev, uint64_t * sse_dev, void * consumer_stream )
{
  if ( !ctx || !streams || !frame_index || !originals || !ssim_dev || n <= 0 ) return fail( AA_ERR_ARGUMENT, "aa_quality_batch_async: bad argument" );
  if ( planes != AA_QUALITY_Y && planes != AA_QUALITY_YUV ) return fail( AA_ERR_ARGUMENT, "aa_quality_batch_async: planes must be 1 (Y) or 3 (Y, U, V), not " + std::to_string( planes ) );
  if ( aa_status st = set_device( ctx ) ) return st;
  for ( int i = 0; i < n; i++ ) {
    const aa_stream * s = streams[i];
    if ( aa_status st = held_decoded_frame( "aa_quality_batch_async", ctx, s, frame_index[i], nullptr ) ) return st;
    const aa_quality_ref & o = originals[i];
    if ( !o.y || ( planes == AA_QUALITY_YUV && ( !o.u || !o.v ) ) ) return fail( AA_ERR_ARGUMENT, "aa_quality_batch_async: null plane in original " + std::to_string( i ) );
    if ( o.y_stride < int64_t( s->pw ) || ( planes == AA_QUALITY_YUV && o.uv_stride < int64_t( s->pw / 2 ) ) )
      return fail( AA_ERR_ARGUMENT, "aa_quality_batch_async: row stride smaller than the padded plane's width in original " + std::to_string( i ) );
  }
  std::vector<QualityPair> pairs;
  pairs.reserve( size_t( n ) * planes );
  for ( int i = 0; i < n; i++ ) {
    aa_stream * s = streams[i];
    const int slot = s->frames[frame_index[i]].out_slot;
    const aa_quality_ref & o = originals[i];
    const void * ob[3] = { o.y, o.u, o.v };
    for ( int p = 0; p < planes; p++ ) {
      const uint32_t w = p ? s->pw / 2 : s->pw, h = p ? s->ph / 2 : s->ph;        // (multiples of 16 / 8: at least one window each way)
      pairs.push_back( { slot_plane( s, slot, p ), w, static_cast<const uint8_t *>( ob[p] ), p ? o.uv_stride : o.y_stride, w, h } );
    }
  }
  return quality_of_planes( ctx, pairs.data(), n * planes, ssim_dev, sse_dev, static_cast<hipStream_t>( consumer_stream ) );
}

} // extern "C"
