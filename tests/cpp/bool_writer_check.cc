// bool_writer.hh against bool_reader.hh, and the host half of the serialisation (serializer.cpp + serialize_common.hh) against frames the
// reference's Frame::serialize wrote.  Stand-alone (its own main; built plain and with -fsanitize=address,undefined by
// tests/test_bool_writer.py):
//
//   bool_writer_check                       generated (bit, probability) sequences through BoolWriter, decoded back with BoolReader and
//                                           BoolReader32: every bit returns; the census of what the sequences exercised is checked too
//                                           (carries that walk back over one, two and more 0xff bytes, probabilities 1 and 255, the empty
//                                           stream, a capacity that is too small: the size needed is still right and no byte beyond it is
//                                           touched)
//   bool_writer_check FILE.ivf[,STATE] ...  every frame of every file: host parser -> records, header, rest of the header, the tables
//                                           before the frame -> serialize_frame_host -> must be the frame's bytes.  STATE: a decoder state
//                                           file in the reference's format that the stream continues from.
//                                           Prints "FILE frames N same M" per file; exit status 1 if any frame of any file differs.
//   bool_writer_check --list FILE.ivf ...   the same, but a file that is not reproduced is only reported (exit status 0): which streams
//                                           parse -> serialise reproduces is a property of the stream, see tests/golden/serialize_fixed_point.json
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../alfalfa_amd/csrc/bool_reader.hh"
#include "../../alfalfa_amd/csrc/bool_writer.hh"
#include "../../alfalfa_amd/csrc/parser.hh"
#include "../../alfalfa_amd/csrc/serializer.hh"

namespace {

struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>( s >> 33 ); } };

struct Census { int sequences = 0, carries = 0, carry1 = 0, carry2 = 0, carry3 = 0, prob1 = 0, prob255 = 0, empty = 0, short_cap = 0; };

// one sequence through the writer (watching for carries: bytes in front of the write position that change), back through both readers
bool round_trip( const std::vector<uint8_t> & bits, const std::vector<uint8_t> & probs, Census & c, const char * what )
{
  const size_t n = bits.size();
  std::vector<uint8_t> buf( n + 16, 0xA5 ), before;
  const uint32_t cap = static_cast<uint32_t>( n + 8 );          // (a bool takes at most 7 bits; the flush four bytes)
  aa::BoolWriter w( buf.data(), cap );
  for ( size_t i = 0; i < n; i++ ) {
    const uint32_t pos = w.size();
    before.assign( buf.begin(), buf.begin() + pos );
    w.put( bits[i], probs[i] );
    int walked = 0;
    for ( uint32_t k = pos; k-- > 0; ) { if ( buf[k] != before[k] ) walked++; else break; }
    if ( walked ) { c.carries++; if ( walked == 1 ) c.carry1++; else if ( walked == 2 ) c.carry2++; else c.carry3++; }
    for ( uint32_t k = 0; k + walked < pos; k++ ) if ( buf[k] != before[k] ) { std::printf( "%s: put %zu changed byte %u, not part of a carry\n", what, i, k ); return false; }
  }
  const uint32_t size = w.finish();
  if ( !w.fits() ) { std::printf( "%s: %zu bools took %u bytes, more than %u\n", what, n, size, cap ); return false; }
  for ( size_t k = cap; k < buf.size(); k++ ) if ( buf[k] != 0xA5 ) { std::printf( "%s: byte %zu beyond the capacity was written\n", what, k ); return false; }
  aa::BoolReader r( buf.data(), size );
  aa::BoolReader32 r32; r32.reset( buf.data(), size );
  for ( size_t i = 0; i < n; i++ ) {
    const int a = r.get( probs[i] ), b = r32.get( probs[i] );
    if ( a != bits[i] || b != bits[i] ) { std::printf( "%s: bool %zu of %zu (probability %u) was %u, read back %d / %d\n", what, i, n, probs[i], bits[i], a, b ); return false; }
  }
  // the same sequence into a range that is too small: the same size is reported, the bytes that fit are the same, nothing beyond is touched
  if ( size > 1 ) {
    const uint32_t small = size / 2;
    std::vector<uint8_t> buf2( size + 8, 0x5A );
    aa::BoolWriter w2( buf2.data(), small );
    for ( size_t i = 0; i < n; i++ ) w2.put( bits[i], probs[i] );
    const uint32_t size2 = w2.finish();
    if ( size2 != size || w2.fits() ) { std::printf( "%s: into %u bytes the writer reports %u bytes, wants %u\n", what, small, size2, size ); return false; }
    for ( size_t k = small; k < buf2.size(); k++ ) if ( buf2[k] != 0x5A ) { std::printf( "%s: byte %zu beyond a capacity of %u was written\n", what, k, small ); return false; }
    c.short_cap++;
  }
  c.sequences++;
  if ( n == 0 ) c.empty++;
  return true;
}

int writer_check()
{
  Census c;
  std::vector<uint8_t> bits, probs;
  if ( !round_trip( bits, probs, c, "empty" ) ) return 1;
  for ( int p : { 1, 255, 128 } )
    for ( int bit = 0; bit < 2; bit++ ) {
      bits.assign( 3000, static_cast<uint8_t>( bit ) ); probs.assign( 3000, static_cast<uint8_t>( p ) );
      if ( p == 1 ) c.prob1++;
      if ( p == 255 ) c.prob255++;
      if ( !round_trip( bits, probs, c, "constant" ) ) return 1;
    }
  // Carries are rare in drawn sequences (the 16 pending bits must all be ones), so they are steered: while the coder's interval
  // [bottom, bottom + range) straddles a byte boundary, the bytes in front of it are pending 0xff; every bool is chosen so that the
  // boundary stays inside (d = its distance from the bottom, 0 < d < range), for `steps` bools, and then a one at a split >= d moves
  // the bottom across: the carry walks back over every 0xff written meanwhile.  The first byte boundary (128 of 255) is inside from
  // the start, so only (range, d) need following, not the writer's state.
  Rng rng { 12345 };
  for ( int steps = 1; steps <= 60; steps++ ) {
    bits.clear(); probs.clear();
    uint32_t range = 255, d = 128;
    for ( int i = 0; i < steps; ) {
      const uint32_t p = 1 + rng.next() % 255, split = 1 + ( ( ( range - 1 ) * p ) >> 8 );
      if ( split == d ) continue;
      if ( split < d ) { bits.push_back( 1 ); d -= split; range -= split; } else { bits.push_back( 0 ); range = split; }
      probs.push_back( static_cast<uint8_t>( p ) );
      const int shift = __builtin_clz( range ) - 24;
      range <<= shift; d <<= shift;
      i++;
    }
    for ( uint32_t p = 1; p < 256; p++ )
      if ( 1 + ( ( ( range - 1 ) * p ) >> 8 ) >= d ) { bits.push_back( 1 ); probs.push_back( static_cast<uint8_t>( p ) ); break; }
    for ( int i = 0; i < 40; i++ ) { const uint32_t r = rng.next(); bits.push_back( r & 1 ); probs.push_back( static_cast<uint8_t>( 1 + ( r >> 1 ) % 255 ) ); }
    if ( !round_trip( bits, probs, c, "steered carry" ) ) return 1;
  }
  for ( int seq = 0; seq < 400; seq++ ) {
    const size_t n = 1 + rng.next() % 4000;
    bits.resize( n ); probs.resize( n );
    const int kind = seq % 4;
    for ( size_t i = 0; i < n; i++ ) {
      const uint32_t r = rng.next();
      uint32_t p, b;
      if ( kind == 0 ) { p = 1 + r % 255; b = ( r >> 8 ) & 1; }                                         // anything
      else if ( kind == 1 ) { p = 1 + r % 255; b = ( ( r >> 8 ) & 255 ) >= p; }                          // what a coder sees: bits drawn with their probability
      else if ( kind == 2 ) { p = ( r & 1 ) ? 255 : 250 + ( r >> 1 ) % 6; b = ( ( r >> 8 ) % 16 ) != 0; } // mostly ones against the odds
      else { p = ( r % 3 == 0 ) ? 1 : ( r % 3 == 1 ? 255 : 128 ); b = ( r >> 8 ) & 1; }                   // the extremes
      bits[i] = static_cast<uint8_t>( b ); probs[i] = static_cast<uint8_t>( p );
    }
    if ( !round_trip( bits, probs, c, "generated" ) ) return 1;
  }
  std::printf( "writer: %d sequences, %d carries (%d over one byte, %d over two, %d over more), %d too-small ranges\n", c.sequences, c.carries, c.carry1, c.carry2, c.carry3, c.short_cap );
  if ( !c.carry1 || !c.carry2 || !c.carry3 || !c.empty || !c.prob1 || !c.prob255 || !c.short_cap ) { std::printf( "writer: the sequences did not exercise every case\n" ); return 1; }
  return 0;
}

bool read_file( const std::string & path, std::vector<uint8_t> & out )
{
  FILE * f = std::fopen( path.c_str(), "rb" );
  if ( !f ) return false;
  std::fseek( f, 0, SEEK_END ); const long n = std::ftell( f ); std::fseek( f, 0, SEEK_SET );
  out.resize( n > 0 ? static_cast<size_t>( n ) : 0 );
  const bool ok = out.empty() || std::fread( out.data(), 1, out.size(), f ) == out.size();
  std::fclose( f );
  return ok;
}

// -> 0 every frame reproduced, 1 some frame differs, 2 the file could not be used
int stream_check( const std::string & arg )
{
  const size_t comma = arg.find( ',' );
  const std::string path = arg.substr( 0, comma );
  std::vector<uint8_t> ivf, state;
  if ( !read_file( path, ivf ) || ivf.size() < 32 || std::memcmp( ivf.data(), "DKIF", 4 ) != 0 ) { std::printf( "%s: not an IVF file\n", path.c_str() ); return 2; }
  const uint16_t w = static_cast<uint16_t>( ivf[12] | ( ivf[13] << 8 ) ), h = static_cast<uint16_t>( ivf[14] | ( ivf[15] << 8 ) );
  aa::Parser parser( w, h );
  try {
    if ( comma != std::string::npos ) {
      if ( !read_file( arg.substr( comma + 1 ), state ) || state.size() < 5 ) { std::printf( "%s: no state file\n", path.c_str() ); return 2; }
      parser.deserialize_reference( state.data() + 5, state.size() - 5 );       // (Decoder::serialize: tag, length, DecoderState, References)
    }
    const size_t nmb = static_cast<size_t>( parser.mb_width() ) * parser.mb_height();
    std::vector<aa_mb_info> mbs( nmb );
    std::vector<int16_t> coeffs( nmb * 25 * 16 );
    std::vector<uint8_t> out;
    int frames = 0, same = 0;
    for ( size_t at = ( ivf[6] | ( ivf[7] << 8 ) ); at + 12 <= ivf.size(); ) {
      const size_t size = ivf[at] | ( ivf[at + 1] << 8 ) | ( ivf[at + 2] << 16 ) | ( static_cast<size_t>( ivf[at + 3] ) << 24 );
      at += 12;
      if ( at + size > ivf.size() ) break;
      uint8_t before[1101];
      const aa::ProbTables & t = parser.probs();
      std::memcpy( before, t.coeff, 1056 ); std::memcpy( before + 1056, t.y_mode, 4 ); std::memcpy( before + 1060, t.uv_mode, 3 ); std::memcpy( before + 1063, t.mv, 38 );
      aa_frame_header hdr;
      aa::Parser again = parser;              // (the state before the frame: what the serialised bytes are parsed from when they differ)
      parser.parse( ivf.data() + at, size, hdr, mbs.data(), coeffs.data() );
      const std::vector<uint8_t> & sub = parser.last_sub_modes();
      aa::serialize_frame_host( hdr, parser.last_header_ext(), before, mbs.data(), coeffs.data(), sub.data(), sub.size(), out );
      const bool eq = out.size() == size && std::memcmp( out.data(), ivf.data() + at, size ) == 0;
      if ( !eq ) {
        size_t d = 0;
        while ( d < out.size() && d < size && out[d] == ivf[at + d] ) d++;
        std::printf( "%s frame %d (%s, %u partitions): %zu bytes, serialised %zu, first difference at byte %zu\n", path.c_str(), frames, hdr.key_frame ? "key" : "inter",
                     hdr.num_dct_partitions, size, out.size(), d );
        // what the serialised frame says instead: the first macroblock whose record differs
        std::vector<aa_mb_info> mbs2( nmb );
        std::vector<int16_t> coeffs2( nmb * 25 * 16 );
        aa_frame_header hdr2;
        try {
          again.parse( out.data(), out.size(), hdr2, mbs2.data(), coeffs2.data() );
          size_t m = 0;
          while ( m < nmb && std::memcmp( &mbs[m], &mbs2[m], sizeof( aa_mb_info ) ) == 0 ) m++;
          if ( m < nmb ) std::printf( "  parsed back: macroblock %zu differs (mode %u / %u, flags %02x / %02x, nz_mask %07x / %07x)\n", m, mbs[m].y_mode, mbs2[m].y_mode, mbs[m].flags,
                                      mbs2[m].flags, mbs[m].nz_mask, mbs2[m].nz_mask );
          else std::printf( "  parsed back: the same records (%u coefficient blocks / %u)\n", hdr.num_coeff_blocks, hdr2.num_coeff_blocks );
        } catch ( const aa::ParseError & e ) { std::printf( "  parsed back: %s\n", e.message.c_str() ); }
      }
      frames++; same += eq;
      at += size;
    }
    std::printf( "%s frames %d same %d\n", path.c_str(), frames, same );
    return same == frames && frames ? 0 : 1;
  } catch ( const aa::ParseError & e ) {
    std::printf( "%s: %s\n", path.c_str(), e.message.c_str() );
    return 2;
  }
}

} // namespace

int main( int argc, char ** argv )
{
  if ( argc == 1 ) return writer_check();
  const bool list = std::strcmp( argv[1], "--list" ) == 0;
  int worst = 0;
  for ( int i = list ? 2 : 1; i < argc; i++ ) {
    const int r = stream_check( argv[i] );
    if ( r > worst && !( list && r == 1 ) ) worst = r;
  }
  return worst ? 1 : 0;
}
