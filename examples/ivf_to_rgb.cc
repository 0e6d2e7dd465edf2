// ivf_to_rgb: the reference's `vp8play` loop (frontend/vp8play.cc) without a window: every shown frame is converted to RGB on the
// GPU -- what VideoDisplay::draw's shader does (display.cc), here through render_rgb / aa_render_rgb_async -- into a device buffer,
// downloaded, and written as raw rgb24 (rawvideo: width x height x 3 bytes per frame, no header).
//
//   ivf_to_rgb [-o out.rgb] input.ivf        (without -o: standard output)
//
//   g++ -std=c++14 -O2 -Iinclude -I$ROCM_PATH/include -D__HIP_PLATFORM_AMD__ examples/ivf_to_rgb.cc -Lalfalfa_amd/lib -lalfalfa_amd
//       -L$ROCM_PATH/lib -lamdhip64 -Wl,-rpath,$PWD/alfalfa_amd/lib:$ROCM_PATH/lib
#define ALFALFA_AMD_GLOBAL_NAMES
#include "alfalfa_amd/alfalfa.hh"

#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

namespace {

void hip_check( const hipError_t e, const char * what )
{
  if ( e != hipSuccess ) throw alfalfa_amd::DeviceError( std::string( what ) + ": " + hipGetErrorString( e ) );
}

// one device buffer of a frame's rgb24 rows, freed with the player loop
struct DeviceFrame
{
  void * p = nullptr;
  explicit DeviceFrame( const size_t bytes ) { hip_check( hipMalloc( &p, bytes ), "hipMalloc" ); }
  ~DeviceFrame() { if ( p ) (void) hipFree( p ); }
  DeviceFrame( const DeviceFrame & ) = delete;
  DeviceFrame & operator=( const DeviceFrame & ) = delete;
};

void play( Player & player, FileDescriptor & sink )
{
  const size_t row = size_t( player.width() ) * 3, bytes = row * player.height();
  DeviceFrame dev( bytes );
  std::vector<uint8_t> host( bytes );
  while ( !player.eof() ) {
    const RasterHandle shown = player.advance();
    alfalfa_amd::render_rgb( { shown }, { aa_rgb_target { dev.p, static_cast<int64_t>( row ), 0 } }, AA_RGB_U8_HWC3 );
    shown.owner()->ctx->sync();
    hip_check( hipMemcpy( host.data(), dev.p, bytes, hipMemcpyDeviceToHost ), "hipMemcpy" );
    sink.write( Chunk( host ) );
  }
}

} // namespace

int main( int argc, char * argv[] )
{
  std::string input, output;
  for ( int i = 1; i < argc; i++ ) {
    if ( !std::strcmp( argv[i], "-o" ) && i + 1 < argc ) output = argv[++i];
    else if ( argv[i][0] != '-' && input.empty() ) input = argv[i];
    else input.clear(), i = argc;
  }
  if ( input.empty() ) {
    std::cerr << "Usage: " << ( argc > 0 ? argv[0] : "ivf_to_rgb" ) << " [-o rgb24_output] input_file\n";
    return EXIT_FAILURE;
  }
  try {
    Player player( input );
    FileDescriptor sink = output.empty() ? FileDescriptor( STDOUT_FILENO ) : FileDescriptor( std::fopen( output.c_str(), "wb" ) );
    play( player, sink );
  } catch ( const std::exception & e ) {
    print_exception( argv[0], e );
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
