// The search rule of alfalfa_amd/csrc/lf_choose.hh, continued over rounds, against the plain loop over all scores (choose_level,
// runtime_lf_search.inc, restated below): generated score sequences across round boundaries for K = 1..8 -- ties, a strictly rising run to
// level_hi, lo == hi, a first score that is not above the start value -- and every range.  Stand-alone: built with the sanitizers and
// run as a program (tests/test_lf_search_fixtures.py); built as a shared library, lf_rule is what that test applies to the oracle's tables.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alfalfa_amd/csrc/lf_choose.hh"

// the reference's choice (encoder.cc:489-503) as aa_stream_lf_search makes it, with the count of candidates it looked at
static void choose_level( const double * q, int n, int level_lo, int * best, double * best_q, int * evaluated )
{
  *best = level_lo; *best_q = -1.0; *evaluated = 0;
  for ( int i = 0; i < n; i++ ) {
    ( *evaluated )++;
    if ( !( q[i] > *best_q ) ) break;
    *best = level_lo + i; *best_q = q[i];
  }
}

// scores[level] for level 0..63; the search over lo..hi in rounds of K; -> rounds run
extern "C" int lf_rule( const double * scores, int lo, int hi, int K, int * best, double * best_score, int * evaluated )
{
  aa::LfChoice c;
  aa::lf_choice_begin( c, lo );
  int rounds = 0;
  for ( int first = lo; !c.done; first += K, rounds++ ) {
    const int n = hi - first + 1 < K ? hi - first + 1 : K;
    if ( n <= 0 ) return -1;                       // (the rule must have ended at level_hi)
    aa::lf_choice_round( c, first, scores + first, n, hi );
  }
  *best = c.best_level; *best_score = c.best_score; *evaluated = c.evaluated;
  return rounds;
}

extern "C" double lf_sse_score_c( uint64_t sse, uint32_t pw, uint32_t ph ) { return aa::lf_sse_score( sse, pw, ph ); }
extern "C" uint32_t lf_segment_levels_c( int enabled, int absolute, const int8_t * lf, int level )
{
  aa::LfSegments s;
  std::memset( &s, 0, sizeof s );
  s.enabled = static_cast<int8_t>( enabled ); s.absolute = static_cast<int8_t>( absolute );
  for ( int k = 0; k < 4; k++ ) s.lf[k] = lf[k];
  return aa::lf_segment_levels( s, level );
}

static int failures = 0;
static long checked = 0;

static void check( const std::vector<double> & scores, const char * what )
{
  for ( int lo = 0; lo < 64; lo++ )
    for ( int hi = lo; hi < 64; hi++ ) {
      int want, want_n; double want_q;
      choose_level( scores.data() + lo, hi - lo + 1, lo, &want, &want_q, &want_n );
      for ( int K = 1; K <= 8; K++ ) {
        int got, got_n; double got_q;
        const int rounds = lf_rule( scores.data(), lo, hi, K, &got, &got_q, &got_n );
        checked++;
        // the rounds: as many as hold the candidates consumed (all of them when the run rises to level_hi)
        const int want_rounds = ( want_n + K - 1 ) / K;
        if ( got != want || got_n != want_n || std::memcmp( &got_q, &want_q, sizeof got_q ) || rounds != want_rounds ) {
          if ( failures++ < 10 )
            std::printf( "%s: levels %d..%d, K %d: level %d score %a after %d candidates in %d rounds, the plain loop gives %d %a %d in %d\n", what, lo, hi, K, got,
                         got_q, got_n, rounds, want, want_q, want_n, want_rounds );
        }
      }
    }
}

int main()
{
  std::vector<double> s( 64 );
  uint32_t seed = 12345u;
  auto next = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  // a strictly rising run to level 63 (the search ends at level_hi, whatever the round)
  for ( int i = 0; i < 64; i++ ) s[i] = 0.25 + i / 256.0;
  check( s, "rising" );
  // strictly falling; constant (a tie does not replace)
  for ( int i = 0; i < 64; i++ ) s[i] = 0.75 - i / 256.0;
  check( s, "falling" );
  for ( int i = 0; i < 64; i++ ) s[i] = 0.5;
  check( s, "constant" );
  // a first score at or below the start value -1: nothing replaces
  for ( int i = 0; i < 64; i++ ) s[i] = i ? 0.5 : -1.0;
  check( s, "first is -1" );
  // a peak at every level, with a tie right after it, then higher scores the rule never sees
  for ( int peak = 0; peak < 64; peak++ ) {
    for ( int i = 0; i < 64; i++ ) s[i] = i <= peak ? 0.1 + i / 128.0 : ( i == peak + 1 ? 0.1 + peak / 128.0 : 0.99 );
    check( s, "peak with a tie" );
  }
  // plateaus and noise: steps of 0, +1 or -1 thousandths
  for ( int round = 0; round < 40; round++ ) {
    double v = 0.5;
    for ( int i = 0; i < 64; i++ ) { const uint32_t r = next() % 4; v += r == 0 ? -0.001 : ( r == 1 ? 0.0 : 0.001 ); s[i] = v; }
    check( s, "noise" );
  }
  // measure 1: the grouping, on values whose quotient is not exact
  const double want = 1.0 - ( 500618.0 / ( 80.0 * 80.0 ) ) / ( 255.0 * 255.0 );
  const double got = aa::lf_sse_score( 500618, 80, 80 );
  if ( std::memcmp( &want, &got, sizeof want ) ) { failures++; std::printf( "lf_sse_score: %a, the formula gives %a\n", got, want ); }
  // segment levels: off, relative with a clamp at both ends, absolute, level 0
  const int8_t lf[4] = { -10, 5, 60, 0 };
  struct { int enabled, absolute, level; uint32_t want; } cases[] = {
    { 0, 0, 21, 0x15151515u }, { 1, 0, 8, 0x08 << 24 | 63u << 16 | 13u << 8 | 0u }, { 1, 1, 8, 0u << 24 | 60u << 16 | 5u << 8 | 0u }, { 1, 1, 0, 0u }, { 0, 0, 0, 0u } };
  for ( const auto & c : cases ) {
    const uint32_t w = lf_segment_levels_c( c.enabled, c.absolute, lf, c.level );
    if ( w != c.want ) { failures++; std::printf( "lf_segment_levels( %d, %d, level %d ): %08x, expected %08x\n", c.enabled, c.absolute, c.level, w, c.want ); }
  }
  std::printf( "%ld searches checked, %d failures\n", checked, failures );
  return failures ? 1 : 0;
}
