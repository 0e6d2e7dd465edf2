// ivf_ssim: the reference's `xc-ssim` loop (frontend/xc-ssim.cc) for two IVF files: the shown frames of both, pair by pair, scored on
// the GPU where they were decoded -- quality_batch / aa_quality_batch_async, a batch of frames at a time -- and one line per frame in
// xc-ssim's format: the SSIM of the luma planes or, with -a, of all three planes separated by tabs.  It stops when either file ends.
//
//   ivf_ssim [-a] a.ivf b.ivf
//
//   g++ -std=c++14 -O2 -Iinclude examples/ivf_ssim.cc -Lalfalfa_amd/lib -lalfalfa_amd -Wl,-rpath,$PWD/alfalfa_amd/lib
#define ALFALFA_AMD_GLOBAL_NAMES
#include "alfalfa_amd/alfalfa.hh"

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

namespace {

constexpr size_t kBatch = 32;      // pairs of frames held in HBM and scored by one call

void score( const std::vector<RasterHandle> & a, const std::vector<RasterHandle> & b, const bool all_planes )
{
  if ( a.empty() ) return;
  for ( const auto & q : alfalfa_amd::quality_batch( a, b, all_planes ) ) {
    std::cout << q[0];
    if ( all_planes ) std::cout << "\t" << q[1] << "\t" << q[2];
    std::cout << std::endl;
  }
}

} // namespace

int main( int argc, char * argv[] )
{
  bool all_planes = false;
  std::vector<std::string> files;
  for ( int i = 1; i < argc; i++ ) {
    if ( !std::strcmp( argv[i], "-a" ) || !std::strcmp( argv[i], "--all-planes" ) ) all_planes = true;
    else if ( argv[i][0] != '-' ) files.push_back( argv[i] );
    else files.clear(), i = argc;
  }
  if ( files.size() != 2 ) {
    std::cerr << "Usage: " << ( argc > 0 ? argv[0] : "ivf_ssim" ) << " [-a] <video1.ivf> <video2.ivf>\n";
    return EXIT_FAILURE;
  }
  try {
    IVFReader first( files[0] ), second( files[1] );
    std::vector<RasterHandle> a, b;
    while ( true ) {
      Optional<RasterHandle> ra = first.get_next_frame(), rb = second.get_next_frame();
      if ( !ra.initialized() || !rb.initialized() ) break;
      a.push_back( ra.get() ); b.push_back( rb.get() );
      if ( a.size() == kBatch ) { score( a, b, all_planes ); a.clear(); b.clear(); }
    }
    score( a, b, all_planes );
  } catch ( const std::exception & e ) {
    print_exception( argv[0], e );
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
