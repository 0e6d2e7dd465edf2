// Host check of alfalfa_amd/csrc/hash_chain.hh: the walker of a job -- the same source a lane of k_hash_chains runs -- against a
// byte-at-a-time loop of the formula.  Built and run by tests/test_hash_chain.py.
//   hash_chain_check                                     the fixed cases; prints "OK <cases>"
//   hash_chain_check segmap W H ABS Q0..Q3 L0..L3 HEX    the segment-map job as the runtime builds it (map: mbw * mbh bytes in hex);
//                                                        prints Segmentation::hash in decimal
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../alfalfa_amd/csrc/hash_chain.hh"

using namespace aa;

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// the formula, one byte at a time, nothing shared with the header
static void plain( uint64_t & seed, uint64_t v ) { seed ^= v + 0x9e3779b9ull + ( seed << 6 ) + ( seed >> 2 ); }
static uint64_t plain_job( const HashJob & j )
{
  uint64_t seed = j.seed_in;
  for ( uint32_t r = 0; r < j.rows; r++ ) {
    for ( uint64_t i = 0; i < j.row_bytes; i++ ) plain( seed, j.src[r * j.row_stride + i] );
    for ( uint32_t i = 0; i < j.pad_per_row; i++ ) plain( seed, j.pad_value );
  }
  for ( uint64_t i = 0; i < j.tail_pad; i++ ) plain( seed, j.pad_value );
  return seed;
}

static long cases = 0;
static void expect( const HashJob & j, const char * what )
{
  const uint64_t got = hash_job_walk( j ), want = plain_job( j );
  if ( got != want ) {
    std::printf( "MISMATCH %s: rows %u row_bytes %llu misalignment %u pad %u tail %llu seed %llx: got %llx want %llx\n", what, j.rows,
                 static_cast<unsigned long long>( j.row_bytes ), static_cast<unsigned>( reinterpret_cast<uintptr_t>( j.src ) & 15 ), j.pad_per_row,
                 static_cast<unsigned long long>( j.tail_pad ), static_cast<unsigned long long>( j.seed_in ), static_cast<unsigned long long>( got ),
                 static_cast<unsigned long long>( want ) );
    std::exit( 1 );
  }
  cases++;
}

static int segmap_mode( int argc, char ** argv )
{
  if ( argc != 14 ) { std::fprintf( stderr, "usage: hash_chain_check segmap W H ABS Q0 Q1 Q2 Q3 L0 L1 L2 L3 HEXMAP\n" ); return 2; }
  const uint32_t w = std::atoi( argv[2] ), h = std::atoi( argv[3] ), mbw = ( w + 15 ) / 16, mbh = ( h + 15 ) / 16;
  uint64_t sh = 0;
  plain( sh, std::atoi( argv[4] ) ? 1 : 0 );
  for ( int i = 0; i < 8; i++ ) plain( sh, static_cast<uint64_t>( static_cast<int64_t>( static_cast<int8_t>( std::atoi( argv[5 + i] ) ) ) ) );
  const char * hex = argv[13];
  if ( std::strlen( hex ) != size_t( 2 ) * mbw * mbh ) { std::fprintf( stderr, "map: expected %u bytes\n", mbw * mbh ); return 2; }
  // (at an odd address, as in the call's pinned buffer, where the maps lie back to back)
  std::vector<uint8_t> store( size_t( mbw ) * mbh + 32 );
  uint8_t * map = store.data() + 16 - ( reinterpret_cast<uintptr_t>( store.data() ) & 15 ) + 5;
  for ( size_t i = 0; i < size_t( mbw ) * mbh; i++ ) { unsigned v = 0; std::sscanf( hex + 2 * i, "%2x", &v ); map[i] = static_cast<uint8_t>( v ); }
  const HashJob j = hash_segment_map_job( map, w, h, mbw, mbh, sh, 0 );
  if ( hash_job_steps( j ) != uint64_t( w ) * h ) { std::fprintf( stderr, "the job has %llu steps, the frame %u x %u pixels\n", static_cast<unsigned long long>( hash_job_steps( j ) ), w, h ); return 1; }
  std::printf( "%llu\n", static_cast<unsigned long long>( hash_job_walk( j ) ) );
  return 0;
}

int main( int argc, char ** argv )
{
  if ( argc > 1 && !std::strcmp( argv[1], "segmap" ) ) return segmap_mode( argc, argv );

  // a 16-byte aligned base with room to move the source by 0 .. 15
  std::vector<uint8_t> store( 4097 + 64 + 120 * 40 );
  uint8_t * base = store.data() + ( 16 - ( reinterpret_cast<uintptr_t>( store.data() ) & 15 ) ) % 16;
  for ( size_t i = 0; base + i < store.data() + store.size(); i++ ) base[i] = static_cast<uint8_t>( rnd() );
  for ( int i = 0; i < 64; i += 3 ) base[i] = static_cast<uint8_t>( 128 + ( rnd() & 127 ) );      // (values >= 128: the byte is zero-extended)
  base[7] = 0xFF; base[16] = 0x80; base[31] = 0xFE;

  // the 1-D form (a raster): every length x every misalignment x two seeds
  const uint64_t lengths[] = { 0, 1, 15, 16, 17, 4097 };
  const uint64_t seeds[] = { 0, 0x0123456789abcdefull };
  for ( uint64_t len : lengths ) for ( int mis = 0; mis < 16; mis++ ) for ( uint64_t seed : seeds ) {
    HashJob j = hash_raster_job( base + mis, len, 0 );
    j.seed_in = seed;
    expect( j, "1-D" );
  }
  // all 0xFF: the largest byte in every position of a 16-byte load
  {
    std::vector<uint8_t> ff( 16 * 5 + 16, 0xFF );
    uint8_t * p = ff.data() + ( 16 - ( reinterpret_cast<uintptr_t>( ff.data() ) & 15 ) ) % 16;
    expect( hash_raster_job( p, 80, 0 ), "0xFF" );
  }
  // the 2-D form (a segment map): rows of 3 and 120 bytes, rows apart by their length, every misalignment of the first row
  for ( uint32_t row_bytes : { 3u, 120u } ) for ( uint32_t pad : { 0u, 30u } ) for ( uint64_t tail : { uint64_t( 0 ), uint64_t( 15 * 33 ) } )
    for ( uint32_t rows : { 1u, 2u, 40u } ) for ( int mis = 0; mis < 16; mis++ ) for ( uint64_t seed : seeds ) {
      HashJob j;
      j.src = base + mis; j.seed_in = seed;
      j.row_bytes = row_bytes; j.row_stride = row_bytes;
      j.rows = rows; j.pad_per_row = pad; j.tail_pad = tail;
      j.out_index = 0; j.pad_value = 3;
      expect( j, "2-D" );
      if ( hash_job_steps( j ) != uint64_t( rows ) * ( row_bytes + pad ) + tail ) { std::printf( "MISMATCH steps\n" ); return 1; }
    }
  // ... and rows further apart than they are long
  {
    HashJob j;
    j.src = base + 1; j.seed_in = 7;
    j.row_bytes = 17; j.row_stride = 23; j.rows = 9; j.pad_per_row = 2; j.tail_pad = 5; j.out_index = 0; j.pad_value = 200;
    expect( j, "stride" );
  }
  // the segment-map job of a 33 x 17 frame (3 x 2 macroblocks: 30 threes behind each map row, 15 x 33 behind the map)
  {
    const HashJob j = hash_segment_map_job( base + 3, 33, 17, 3, 2, 99, 0 );
    if ( j.rows != 2 || j.row_bytes != 3 || j.pad_per_row != 30 || j.tail_pad != 15 * 33 || j.pad_value != 3 ) { std::printf( "MISMATCH segment-map job fields\n" ); return 1; }
    expect( j, "segment map" );
  }
  std::printf( "OK %ld\n", cases );
  return 0;
}
