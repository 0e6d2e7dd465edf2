// RasterHandle::quality and quality_batch against the host measure: for every pair of shown frames of two IVF files, the SSIM computed
// on the device from the two handles equals VP8Raster::quality / ssim( Plane, Plane ) of their downloads exactly.
//   quality_handles a.ivf b.ivf   -> "N pairs equal" on standard output, exit status 0; the first difference otherwise
#define ALFALFA_AMD_GLOBAL_NAMES
#include "alfalfa_amd/alfalfa.hh"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main( int argc, char * argv[] )
{
  if ( argc != 3 ) { std::fprintf( stderr, "Usage: %s a.ivf b.ivf\n", argc > 0 ? argv[0] : "quality_handles" ); return EXIT_FAILURE; }
  try {
    IVFReader first( argv[1] ), second( argv[2] );
    std::vector<RasterHandle> a, b;
    while ( true ) {
      Optional<RasterHandle> ra = first.get_next_frame(), rb = second.get_next_frame();
      if ( !ra.initialized() || !rb.initialized() ) break;
      a.push_back( ra.get() ); b.push_back( rb.get() );
    }
    if ( a.empty() ) { std::fprintf( stderr, "no frames\n" ); return EXIT_FAILURE; }
    std::vector<double> single;
    for ( size_t i = 0; i < a.size(); i++ ) single.push_back( a[i].quality( b[i] ) );     // (before anything is downloaded)
    const auto luma = alfalfa_amd::quality_batch( a, b ), all = alfalfa_amd::quality_batch( a, b, true );
    for ( size_t i = 0; i < a.size(); i++ ) {
      const VP8Raster & x = a[i].get(), & y = b[i].get();
      const double want[3] = { x.quality( y ), ssim( x.U(), y.U() ), ssim( x.V(), y.V() ) };
      if ( single[i] != want[0] || luma[i][0] != want[0] || luma[i][1] != 0.0 || luma[i][2] != 0.0
           || all[i][0] != want[0] || all[i][1] != want[1] || all[i][2] != want[2] ) {
        std::fprintf( stderr, "pair %zu: device %.17g | %.17g %.17g %.17g, host %.17g %.17g %.17g\n", i, single[i], all[i][0], all[i][1], all[i][2],
                      want[0], want[1], want[2] );
        return EXIT_FAILURE;
      }
      if ( b[i].quality( a[i] ) != want[0] ) { std::fprintf( stderr, "pair %zu: not symmetric\n", i ); return EXIT_FAILURE; }
    }
    std::printf( "%zu pairs equal\n", a.size() );
  } catch ( const std::exception & e ) {
    print_exception( argv[0], e );
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
