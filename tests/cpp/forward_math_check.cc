// Test program (not product code): the forward transforms and the quantiser of alfalfa_amd/csrc/vp8_math.hh -- the source the rebase
// kernels compile for the device -- compiled for the host and pinned to a table of inputs and outputs that tests/rebase_model.py
// produced (tests/test_forward_math.py writes it to stdin).  Lines:
//   D r0 .. r15 c0 .. c15     residual block (rows) -> forward DCT, raster order      (fdct_pass1 per row, fdct_pass2 per column)
//   W d0 .. d15 y0 .. y15     16 luma DCs (raster) -> forward WHT                      (fwht_pass1 per row, fwht_pass2 per column)
//   Q n f q                   numerator, factor -> quotient truncated toward zero
// Prints "OK <lines checked>" or the first line that differs.
#include <cstdio>
#include <cstring>

#include "../../alfalfa_amd/csrc/vp8_math.hh"

static void fdct( const int * r, int * c )
{
  int im[16];
  for ( int i = 0; i < 4; i++ ) { const aa::Quad v = aa::fdct_pass1( r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3] ); im[4 * i] = v.v0; im[4 * i + 1] = v.v1; im[4 * i + 2] = v.v2; im[4 * i + 3] = v.v3; }
  for ( int i = 0; i < 4; i++ ) { const aa::Quad v = aa::fdct_pass2( im[i], im[i + 4], im[i + 8], im[i + 12] ); c[i] = v.v0; c[i + 4] = v.v1; c[i + 8] = v.v2; c[i + 12] = v.v3; }
}

static void fwht( const int * d, int * y )
{
  int im[16];
  for ( int i = 0; i < 4; i++ ) { const aa::Quad v = aa::fwht_pass1( d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3] ); im[4 * i] = v.v0; im[4 * i + 1] = v.v1; im[4 * i + 2] = v.v2; im[4 * i + 3] = v.v3; }
  for ( int i = 0; i < 4; i++ ) { const aa::Quad v = aa::fwht_pass2( im[i], im[i + 4], im[i + 8], im[i + 12] ); y[i] = v.v0; y[i + 4] = v.v1; y[i + 8] = v.v2; y[i + 12] = v.v3; }
}

int main()
{
  char kind;
  long checked = 0;
  while ( std::scanf( " %c", &kind ) == 1 ) {
    if ( kind == 'Q' ) {
      int n, f, q;
      if ( std::scanf( "%d %d %d", &n, &f, &q ) != 3 ) { std::printf( "bad Q line %ld\n", checked ); return 2; }
      if ( aa::quantize( n, f ) != q ) { std::printf( "line %ld: quantize( %d, %d ) = %d, the model says %d\n", checked, n, f, aa::quantize( n, f ), q ); return 1; }
    } else if ( kind == 'D' || kind == 'W' ) {
      int in[16], want[16], got[16];
      for ( int & v : in ) if ( std::scanf( "%d", &v ) != 1 ) { std::printf( "bad %c line %ld\n", kind, checked ); return 2; }
      for ( int & v : want ) if ( std::scanf( "%d", &v ) != 1 ) { std::printf( "bad %c line %ld\n", kind, checked ); return 2; }
      if ( kind == 'D' ) fdct( in, got ); else fwht( in, got );
      if ( std::memcmp( got, want, sizeof got ) != 0 ) {
        std::printf( "line %ld (%c): input", checked, kind );
        for ( int v : in ) std::printf( " %d", v );
        std::printf( "\n  vp8_math.hh" );
        for ( int v : got ) std::printf( " %d", v );
        std::printf( "\n  the model  " );
        for ( int v : want ) std::printf( " %d", v );
        std::printf( "\n" );
        return 1;
      }
    } else { std::printf( "unknown line kind %c\n", kind ); return 2; }
    checked++;
  }
  std::printf( "OK %ld\n", checked );
  return 0;
}
