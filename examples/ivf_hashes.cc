// ivf-hashes: N IVF files (any frame sizes) decoded in LOCK STEP, as decode_many does, and after every frame index the DecoderHash
// of every decoder still running -- what `cout << player` prints in the reference (player.cc:75-78) -- with ONE
// Decoder::prefetch_hashes per frame index: every raster and segment map that has no cached hash is a chain of one kernel, a GPU
// lane each, and nothing is downloaded.  One line per file and frame:  <file> <frame> <hash> (<state>_<last>_<golden>_<alternative>)
//   g++ -std=c++14 -O2 -Iinclude examples/ivf_hashes.cc -Lalfalfa_amd/lib -lalfalfa_amd -Wl,-rpath,$PWD/alfalfa_amd/lib
#define ALFALFA_AMD_GLOBAL_NAMES
#include "alfalfa_amd/alfalfa.hh"

#include <iostream>

using namespace std;

int main( int argc, char * argv[] )
{
  try {
    if ( argc < 2 ) { cerr << "Usage: " << argv[0] << " input.ivf...\n"; return EXIT_FAILURE; }

    vector<IVF> files;
    vector<unique_ptr<FramePlayer>> players;
    vector<unsigned int> next;                      // next frame of each file
    for ( int i = 1; i < argc; i++ ) {
      files.emplace_back( argv[i] );
      if ( files.back().fourcc() != "VP80" ) throw Unsupported( "not a VP8 file" );
      players.emplace_back( new FramePlayer( files.back().width(), files.back().height() ) );
      unsigned int first = 0;                       // start at the first key frame, like FilePlayer (player.cc:96-105)
      while ( first < files.back().frame_count() and ( files.back().frame( first ).octet() & 1 ) ) first++;
      next.push_back( first );
    }

    while ( true ) {
      vector<Decoder *> decoders; vector<Chunk> frames; vector<size_t> who;
      for ( size_t i = 0; i < files.size(); i++ ) {
        if ( next[i] >= files[i].frame_count() ) continue;
        decoders.push_back( &players[i]->mutable_decoder() ); frames.push_back( files[i].frame( next[i]++ ) ); who.push_back( i );
      }
      if ( decoders.empty() ) break;
      Decoder::get_frame_outputs( decoders, frames );
      Decoder::prefetch_hashes( decoders );         // one kernel for all of them; the lines below read the caches
      for ( size_t k = 0; k < decoders.size(); k++ ) cout << argv[1 + who[k]] << " " << next[who[k]] - 1 << " " << *players[who[k]] << "\n";
    }
  } catch ( const exception & e ) {
    print_exception( argv[0], e );
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
