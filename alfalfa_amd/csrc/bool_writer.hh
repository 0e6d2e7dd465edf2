// VP8 boolean entropy ENCODER, host and device (one source): the writing half of bool_reader.hh / BoolReader32.
//
// Same arithmetic as the reference's BoolEncoder (bool_encoder.hh:60-152, RFC 6386 section 7 with libvpx's normalisation):
// split = 1 + (((range-1)*prob)>>8), a 1 moves the bottom of the interval up by split, the range is shifted back above 127 and
// every eighth shifted bit completes a byte; a carry out of the 24 bits kept walks BACK over the bytes already written (0xff
// becomes 0x00 until a byte takes the one); finish() is the reference's flush: 32 zeros at probability 128, which pushes the
// last four bytes of the interval out (what libvpx's vp8_stop_encode does, not the RFC's shorter flush).
//
// The writer owns [out, out + capacity): a byte that has no room is counted and not stored, and a carry never touches a byte at or
// beyond the capacity -- so size() is the size the stream NEEDS whether it fitted or not, and nothing outside the range is written.
// A carry only ever changes bytes this writer stored earlier: on the GPU every lane has a range of its own and uses plain byte
// stores and loads of its own bytes.
#pragma once
#include <stdint.h>

#if defined( __HIPCC__ )
#define AA_BW_HD __host__ __device__ inline __attribute__( ( always_inline ) )
#else
#define AA_BW_HD inline
#endif

namespace aa {

class BoolWriter
{
  uint8_t * out_ = nullptr;
  uint32_t cap_ = 0, pos_ = 0;
  uint32_t range_ = 255, bottom_ = 0;
  int count_ = -24;

  AA_BW_HD void add_one()          // BoolEncoder::add_one_to_output
  {
    if ( pos_ > cap_ ) return;     // (the stream did not fit: its bytes are not all there, and it is refused anyway)
    uint32_t x = pos_;
    while ( x > 0 && out_[x - 1] == 255 ) out_[--x] = 0;
    if ( x > 0 ) out_[x - 1] = static_cast<uint8_t>( out_[x - 1] + 1 );
  }

public:
  AA_BW_HD BoolWriter() {}
  AA_BW_HD BoolWriter( uint8_t * out, uint32_t capacity ) : out_( out ), cap_( capacity ) {}

  AA_BW_HD void put( const int bit, const uint32_t prob = 128 )
  {
    const uint32_t split = 1 + ( ( ( range_ - 1 ) * prob ) >> 8 );
    if ( bit ) { bottom_ += split; range_ -= split; }
    else range_ = split;
    int shift = __builtin_clz( range_ ) - 24;          // vp8_norm[range]: range in [1, 255]
    range_ <<= shift;
    count_ += shift;
    if ( count_ >= 0 ) {
      const int offset = shift - count_;
      if ( ( bottom_ << ( offset - 1 ) ) & 0x80000000u ) add_one();
      if ( pos_ < cap_ ) out_[pos_] = static_cast<uint8_t>( bottom_ >> ( 24 - offset ) );
      pos_++;
      bottom_ <<= offset;
      shift = count_;
      bottom_ &= 0xFFFFFFu;
      count_ -= 8;
    }
    bottom_ <<= shift;
  }

  AA_BW_HD void literal( const uint32_t v, int bits ) { while ( bits-- ) put( ( v >> bits ) & 1u ); }      // Unsigned<width>: MSB first
  AA_BW_HD void signed_literal( const int v, const int bits ) { literal( static_cast<uint32_t>( v < 0 ? -v : v ), bits ); put( v < 0 ); }   // Signed<width>

  // BoolEncoder::finish -> the bytes the stream takes (more than the capacity: it did not fit)
  AA_BW_HD uint32_t finish()
  {
    for ( int i = 0; i < 32; i++ ) put( 0 );
    return pos_;
  }
  AA_BW_HD uint32_t size() const { return pos_; }
  AA_BW_HD bool fits() const { return pos_ <= cap_; }
};

} // namespace aa
