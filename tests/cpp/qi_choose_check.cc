// The search rule of alfalfa_amd/csrc/qi_choose.hh, continued one candidate at a time, against the plain loop of
// Encoder::encode_with_target_size (encoder.cc:597-628, restated below): every range 0 <= lo <= hi <= 127, targets below, inside and above
// the size table, size tables that fall with the index (what an encoder gives), that rise, that are constant and that are noise -- the
// choice, the number of estimates and the candidates visited, in order.  And the starting range (encoder.cc:597-608) over every last
// index.  Stand-alone: built with the sanitizers and run as a program (tests/test_qi_choose.py); built as a shared library, qi_rule is
// what the fixture tests apply to size tables.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../alfalfa_amd/csrc/qi_choose.hh"

// the reference's loop, as written there; visited[]: the y_qi of every estimate
static int plain_loop( const uint64_t * sizes, int y_qi_min, int y_qi_max, uint64_t target_size, int * visited, int * n_visited )
{
  uint8_t best_y_qi = std::numeric_limits<uint8_t>::max();
  uint64_t estimated_size = target_size;
  *n_visited = 0;
  while ( y_qi_min <= y_qi_max ) {
    uint64_t y_qi = ( y_qi_min + y_qi_max ) / 2;
    estimated_size = sizes[y_qi];
    visited[( *n_visited )++] = static_cast<int>( y_qi );
    if ( estimated_size <= target_size or ( y_qi_min == y_qi_max and best_y_qi == std::numeric_limits<uint8_t>::max() ) ) {
      best_y_qi = static_cast<uint8_t>( y_qi );
      y_qi_max = static_cast<int>( y_qi ) - 1;
    }
    else if ( estimated_size > target_size ) {
      y_qi_min = static_cast<int>( y_qi ) + 1;
    }
  }
  return best_y_qi;
}

// sizes[q] for q 0..127; the search over lo..hi; visited: room for 8 -> the choice; *steps = estimates made
extern "C" int qi_rule( const uint64_t * sizes, int lo, int hi, uint64_t target, int * visited, int * steps )
{
  aa::QiChoice c;
  aa::qi_choice_begin( c, lo, hi );
  while ( !aa::qi_choice_done( c ) ) {
    if ( c.steps >= 8 ) return -1;
    const int q = aa::qi_choice_candidate( c );
    visited[c.steps] = q;
    aa::qi_choice_step( c, sizes[q], target );
  }
  *steps = c.steps;
  return c.best;
}

extern "C" void qi_range( int last_q, int * lo, int * hi ) { aa::qi_target_range( last_q, *lo, *hi ); }

static int failures = 0;
static long checked = 0;

static void check( const std::vector<uint64_t> & sizes, const char * what )
{
  uint64_t smallest = sizes[0], largest = sizes[0];
  for ( uint64_t s : sizes ) { smallest = s < smallest ? s : smallest; largest = s > largest ? s : largest; }
  std::vector<uint64_t> targets = { 0, smallest ? smallest - 1 : 0, smallest, largest, largest + 1, ~0ull };
  for ( int q = 0; q < 128; q += 9 ) { targets.push_back( sizes[q] ); targets.push_back( sizes[q] + 1 ); if ( sizes[q] ) targets.push_back( sizes[q] - 1 ); }
  for ( int lo = 0; lo < 128; lo++ )
    for ( int hi = lo; hi < 128; hi++ )
      for ( uint64_t target : targets ) {
        int want_v[128], want_n, got_v[8], got_n = 0;
        const int want = plain_loop( sizes.data(), lo, hi, target, want_v, &want_n );
        const int got = qi_rule( sizes.data(), lo, hi, target, got_v, &got_n );
        checked++;
        bool same = got == want && got_n == want_n && want_n <= ( lo >= 4 ? 7 : aa::kQiMaxSteps ) && want >= lo && want <= hi;
        for ( int i = 0; same && i < want_n; i++ ) same = got_v[i] == want_v[i];
        if ( !same && failures++ < 10 )
          std::printf( "%s: range %d..%d, target %llu: %d after %d estimates, the plain loop gives %d after %d\n", what, lo, hi, static_cast<unsigned long long>( target ), got, got_n,
                       want, want_n );
      }
}

int main()
{
  std::vector<uint64_t> s( 128 );
  uint32_t seed = 2463534242u;
  auto next = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  for ( int q = 0; q < 128; q++ ) s[q] = 16ull * ( 40000 / ( q + 2 ) );          // falling, as an encoder's sizes fall
  check( s, "falling" );
  for ( int q = 0; q < 128; q++ ) s[q] = 16ull * ( 100 + 7 * q );                // rising
  check( s, "rising" );
  for ( int q = 0; q < 128; q++ ) s[q] = 4800;                                   // constant: every candidate ties with a target of 4800
  check( s, "constant" );
  for ( int round = 0; round < 6; round++ ) {                                    // falling with plateaus and bumps: not monotone
    uint64_t v = 90000;
    for ( int q = 0; q < 128; q++ ) { const uint32_t r = next() % 5; v = r == 0 ? v + 320 : ( r == 1 ? v : v - 160 * ( r - 1 ) ); s[q] = v; }
    check( s, "bumpy" );
  }
  for ( int round = 0; round < 3; round++ ) {                                    // noise
    for ( int q = 0; q < 128; q++ ) s[q] = 16ull * ( next() % 4096 );
    check( s, "noise" );
  }
  // the starting range: encoder.cc:597-608 as written
  for ( int last = -1; last < 128; last++ ) {
    int y_qi_min = 4, y_qi_max = 127;
    if ( last >= 0 ) {
      const int radius = 16;
      if ( last - radius >= y_qi_min ) y_qi_min = last - radius;
      y_qi_max = y_qi_max < last + radius ? y_qi_max : last + radius;
    }
    int lo, hi;
    qi_range( last, &lo, &hi );
    if ( lo != y_qi_min || hi != y_qi_max || lo > hi ) { failures++; std::printf( "range after %d: %d..%d, the reference gives %d..%d\n", last, lo, hi, y_qi_min, y_qi_max ); }
  }
  std::printf( "%ld searches checked, %d failures\n", checked, failures );
  return failures ? 1 : 0;
}
