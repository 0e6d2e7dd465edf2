// Decoder::prefetch_hashes against the per-decoder route: two IVF files, each decoded by two decoders in lock step; after every frame
// index one pair is prefetched (one kernel for both decoders), the other never is.  get_hash(), minihash(), the references
// (RasterHandle::operator==: by hash) and the decoders themselves must compare equal across the pairs, a second prefetch must launch
// no raster chain, and minihash_match must hold against the twin's value.
//   prefetch_hashes_check a.ivf b.ivf   -> "N frame indices equal" on standard output, exit status 0; the first difference otherwise
#define ALFALFA_AMD_GLOBAL_NAMES
#include "alfalfa_amd/alfalfa.hh"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

int main( int argc, char * argv[] )
{
  if ( argc != 3 ) { std::fprintf( stderr, "Usage: %s a.ivf b.ivf\n", argc > 0 ? argv[0] : "prefetch_hashes_check" ); return EXIT_FAILURE; }
  try {
    std::vector<IVF> files;
    std::vector<std::unique_ptr<Decoder>> fetched, plain;
    for ( int i = 1; i < argc; i++ ) {
      files.emplace_back( argv[i] );
      fetched.emplace_back( new Decoder( files.back().width(), files.back().height() ) );
      plain.emplace_back( new Decoder( files.back().width(), files.back().height() ) );
    }
    aa_ctx * const ctx = alfalfa_amd::GpuContext::process_default()->get();
    unsigned int t = 0;
    for ( ; ; t++ ) {
      std::vector<Decoder *> a, b; std::vector<Chunk> frames;
      for ( size_t i = 0; i < files.size(); i++ ) {
        if ( t >= files[i].frame_count() ) continue;
        a.push_back( fetched[i].get() ); b.push_back( plain[i].get() ); frames.push_back( files[i].frame( t ) );
      }
      if ( a.empty() ) break;
      Decoder::get_frame_outputs( a, frames );
      Decoder::get_frame_outputs( b, frames );
      uint64_t before[4], first[4], second[4];
      alfalfa_amd::check( aa_ctx_hash_stats( ctx, before, 0 ) );
      Decoder::prefetch_hashes( a );
      alfalfa_amd::check( aa_ctx_hash_stats( ctx, first, 0 ) );
      Decoder::prefetch_hashes( a );
      alfalfa_amd::check( aa_ctx_hash_stats( ctx, second, 0 ) );
      if ( t == 0 && first[0] == before[0] ) { std::fprintf( stderr, "the prefetch launched no chain for the key frames\n" ); return EXIT_FAILURE; }
      // (rasters are cached per raster; a segment map is hashed anew by every call: one chain per decoder with segmentation on)
      uint64_t maps = 0;
      for ( const Decoder * d : a ) if ( d->get_state().segmentation.initialized() ) maps++;
      if ( second[0] - first[0] != maps || second[3] != first[3] ) {
        std::fprintf( stderr, "frame %u: the second prefetch launched %llu chains for %llu segment maps and filled %llu cache entries\n", t,
                      static_cast<unsigned long long>( second[0] - first[0] ), static_cast<unsigned long long>( maps ), static_cast<unsigned long long>( second[3] - first[3] ) );
        return EXIT_FAILURE;
      }
      for ( size_t k = 0; k < a.size(); k++ ) {
        const DecoderHash ha = a[k]->get_hash(), hb = b[k]->get_hash();
        if ( !( ha == hb ) || ha.hash() != hb.hash() ) { std::fprintf( stderr, "frame %u decoder %zu: %s != %s\n", t, k, ha.str().c_str(), hb.str().c_str() ); return EXIT_FAILURE; }
        if ( a[k]->minihash() != b[k]->minihash() || !a[k]->minihash_match( b[k]->minihash() ) ) { std::fprintf( stderr, "frame %u decoder %zu: minihash\n", t, k ); return EXIT_FAILURE; }
        const References ra = a[k]->get_references(), rb = b[k]->get_references();
        if ( !( ra.last == rb.last ) || !( ra.golden == rb.golden ) || !( ra.alternative == rb.alternative ) ) { std::fprintf( stderr, "frame %u decoder %zu: references differ\n", t, k ); return EXIT_FAILURE; }
        if ( *a[k] != *b[k] ) { std::fprintf( stderr, "frame %u decoder %zu: decoders differ\n", t, k ); return EXIT_FAILURE; }
      }
      if ( a.size() == 2 && *a[0] == *b[1] ) { std::fprintf( stderr, "frame %u: decoders of different files compare equal\n", t ); return EXIT_FAILURE; }
    }
    if ( t == 0 ) { std::fprintf( stderr, "no frames\n" ); return EXIT_FAILURE; }
    std::printf( "%u frame indices equal\n", t );
  } catch ( const std::exception & e ) {
    print_exception( argv[0], e );
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
