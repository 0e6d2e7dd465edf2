// One macroblock of the re-encode (aa_reencode_batch) by sixteen lanes: the pixel side of reencode_search.hh's decision -- SAD, variance,
// the B_PRED trial -- and the chosen mode applied as the rebase applies it (rebase_inl.hh).  Written once for the kernel and for the
// host simulation: `Lanes` says what "every lane b does f" and "the sum over the lanes" mean.  k_reencode_inter (reencode_kernels.hip)
// gives a lane's own registers and a shuffle reduction; tests/cpp/reencode_sim.cc gives sixteen register files and a loop.  Between
// two phases that talk through the slot's LDS picture stands lanes.sync().
//
//   Lanes::each( f )     f( b, regs of lane b ) for b = 0..15
//   Lanes::sum( f )      the sum of f( b, regs ) over the sixteen lanes (uint32_t), known to every lane;  sumi: the same, signed
//   Lanes::sync()        what lanes stored into the slot's ReencLds before it is visible to all of them after it
#pragma once
#include "rebase_inl.hh"
#include "reencode_search.hh"

namespace aa {
namespace {

struct alignas( 16 ) ReencLds {
  RebaseIntraLds L;
  alignas( 4 ) uint8_t bm[16];     // the sub-block modes the B_PRED trial chose (zero where it did not run)
  uint32_t trial_mask;             // ... and which of its sub-blocks kept a coefficient
};

struct ReencRegs {
  int t[16];                       // the lane's 4x4 luma block of the target
  int p[16], q[16];                // applying a mode: the lane's prediction and quantised coefficients
  int32_t s0; uint32_t s1;         // partial sums on their way to Lanes::sum
  bool nz, nz2;
};

// The second pass's (Key2Policy; k_encode_key2's lanes and tests/cpp/encode2_sim.cc's): the lane's trellis between its build and its walk
struct ReencRegs2 : ReencRegs {
  Trellis tr;
};

// The Y2 block of a macroblock in the second pass, in the steps the trellis stands between: the forward WHT of the 16 luma DCs (raster
// order, in LDS) -> c, unquantised; and the decoder's way back from the quantised block -- dequantise, inverse WHT -- to the DC luma
// block b is reconstructed with (the statements of rebase_inl.hh's y2_block).
AA_MHD void y2_forward( const int16_t * dcs, int ( &c )[16] )
{
  int w1[16];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int i = 0; i < 4; i++ ) { const Quad v = fwht_pass1( dcs[4 * i], dcs[4 * i + 1], dcs[4 * i + 2], dcs[4 * i + 3] ); w1[4 * i] = v.v0; w1[4 * i + 1] = v.v1; w1[4 * i + 2] = v.v2; w1[4 * i + 3] = v.v3; }
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int i = 0; i < 4; i++ ) { const Quad v = fwht_pass2( w1[i], w1[i + 4], w1[i + 8], w1[i + 12] ); c[i] = v.v0; c[i + 4] = v.v1; c[i + 8] = v.v2; c[i + 12] = v.v3; }
}
AA_MHD int y2_back( const int ( &q2 )[16], const uint16_t * quant, const int b )
{
  int c[16], im[16];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int i = 0; i < 16; i++ ) c[i] = dequant( q2[i], i == 0 ? quant[Q_Y2_DC] : quant[Q_Y2_AC] );
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int i = 0; i < 4; i++ ) { const Quad v = iwht_pass1( c[i], c[i + 4], c[i + 8], c[i + 12] ); im[i] = v.v0; im[i + 4] = v.v1; im[i + 8] = v.v2; im[i + 12] = v.v3; }
  int dc_back = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
  for ( int i = 0; i < 4; i++ ) {
    const Quad v = iwht_pass2( im[4 * i], im[4 * i + 1], im[4 * i + 2], im[4 * i + 3] );
    dc_back = b == 4 * i ? v.v0 : dc_back; dc_back = b == 4 * i + 1 ? v.v1 : dc_back;
    dc_back = b == 4 * i + 2 ? v.v2 : dc_back; dc_back = b == 4 * i + 3 ? v.v3 : dc_back;
  }
  return static_cast<int16_t>( dc_back );
}

// P: whose decision this is (reencode_search.hh) -- the re-encode's, or the forward encoder's for an inter or a key frame
template <class Lanes, class P = ReencodePolicy>
struct ReencMb {
  Lanes & lanes;
  const aa_reencode_dev_job & RJ;
  const aa_rebase_dev_job & J;
  const typename P::Costs & C;
  ReencLds & S;
  const size_t mi;
  const int col, row, pw, ph, cw, ch, x0, y0;
  ReencNeighbour above, left;
  uint32_t above_mask = 0, left_mask = 0;      // the second pass: which blocks of the macroblocks above and to the left hold a coefficient

  AA_MHD ReencMb( Lanes & l, const aa_reencode_dev_job & j, ReencLds & s, const size_t m )
    : lanes( l ), RJ( j ), J( j.base ), C( *static_cast<const typename P::Costs *>( j.costs ) ), S( s ), mi( m ), col( static_cast<int>( m % j.base.mbw ) ),
      row( static_cast<int>( m / j.base.mbw ) ), pw( j.base.mbw * 16 ), ph( j.base.mbh * 16 ), cw( j.base.mbw * 8 ), ch( j.base.mbh * 8 ), x0( col * 16 ), y0( row * 16 )
  {}

  // Where the macroblock's original, its search and its candidates' predictions lie, and how large the reference planes are.  A frame
  // encoded whole: where the macroblock itself lies, in planes of the frame's size.  The size estimate (P::kSampled; Encoder::estimate_size,
  // size_estimation.cc): the job's frame is the small one, macroblock (col, row) of it stands for the original's (4 col, 4 row) -- the
  // original is read there and the candidates predict from there (reference.macroblock( original_mb.Y.column(), .. ), encode_inter.cc:184,
  // 254,448) -- while the census, the clamp, the intra neighbours and the reconstruction are the small frame's at (col, row).
  AA_MHD int tx() const { if constexpr ( P::kSampled ) return x0 * 4; else return x0; }
  AA_MHD int ty() const { if constexpr ( P::kSampled ) return y0 * 4; else return y0; }
  AA_MHD int tcx() const { if constexpr ( P::kSampled ) return col * 32; else return col * 8; }      // (the same in the chroma planes)
  AA_MHD int tcy() const { if constexpr ( P::kSampled ) return row * 32; else return row * 8; }
  AA_MHD int rw() const { if constexpr ( P::kSampled ) return P::full_mbw( C ) * 16; else return pw; }
  AA_MHD int rh() const { if constexpr ( P::kSampled ) return P::full_mbh( C ) * 16; else return ph; }

  // a neighbour's side record: written by another wave of the workgroup in an earlier round, read past the CU's L1
  AA_MHD ReencNeighbour neighbour( const size_t at ) const
  {
    const uint8_t * p = reinterpret_cast<const uint8_t *>( RJ.nb + at * 4 );
    ReencNeighbour n;
    n.mv = load_recon_u32( p ); n.inter = load_recon_u32( p + 4 ); n.bm_bottom = load_recon_u32( p + 8 ); n.bm_right = load_recon_u32( p + 12 );
    return n;
  }

  // The four pixels above and to the right of the macroblock (the above-right predictor of its fourth sub-block column): beyond the
  // raster's last column the pixel to their left is replicated.  The estimate's reconstruction raster is the ORIGINAL's size with only
  // the small frame's corner written (size_estimation.cc:56,119): beyond the small frame's last column, but inside the raster, lie pixels
  // no estimate writes -- zero in a raster fresh from the allocator, and zero here.
  AA_MHD bool above_right_beyond_raster() const { if constexpr ( P::kSampled ) return col + 1 >= P::full_mbw( C ); else return x0 + 16 >= pw; }
  AA_MHD bool above_right_unwritten() const { if constexpr ( P::kSampled ) return x0 + 16 >= pw; else return false; }
  // (what they hold is the policy's to say: 0 under the product's two, reencode_search.hh)
  AA_MHD uint32_t unwritten_pixels() const { if constexpr ( P::kSampled ) return P::unwritten_pixels( C, row ); else return 0; }

  // the lane's target block, and the slot's picture of the neighbourhood (the layout of k_rebase_intra, staged by sixteen lanes)
  AA_MHD void stage()
  {
    const uint8_t * Y = J.recon[0];
    lanes.each( [&]( const int b, ReencRegs & R ) {
      const uint8_t * t = J.target[0] + static_cast<int64_t>( ty() + ( b >> 2 ) * 4 ) * J.target_stride[0] + tx() + ( b & 3 ) * 4;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
      for ( int i = 0; i < 16; i++ ) R.t[i] = t[( i >> 2 ) * J.target_stride[0] + ( i & 3 )];
      if ( b < 6 ) {
        uint32_t v;
        if ( y0 == 0 ) v = 0x7F7F7F7Fu;
        else if ( b == 0 ) v = x0 > 0 ? load_recon_u32( Y + static_cast<size_t>( y0 - 1 ) * pw + x0 - 4 ) : 0x81818181u;
        else if ( b <= 4 ) v = load_recon_u32( Y + static_cast<size_t>( y0 - 1 ) * pw + x0 + ( b - 1 ) * 4 );
        else if ( above_right_beyond_raster() ) v = 0x01010101u * ( load_recon_u32( Y + static_cast<size_t>( y0 - 1 ) * pw + pw - 4 ) >> 24 );   // replicate: prediction.cc:144-151
        else if ( above_right_unwritten() ) v = unwritten_pixels();
        else v = load_recon_u32( Y + static_cast<size_t>( y0 - 1 ) * pw + x0 + 16 );
        *reinterpret_cast<uint32_t *>( &S.L.y[0][b * 4] ) = v;
      } else if ( b < 12 ) {
        const int pl = ( b - 6 ) / 3, l = ( b - 6 ) % 3, cx0 = col * 8, cy0 = row * 8;
        const uint8_t * Cp = J.recon[1 + pl];
        uint32_t v;
        if ( cy0 == 0 ) v = 0x7F7F7F7Fu;
        else if ( l == 0 ) v = cx0 > 0 ? load_recon_u32( Cp + static_cast<size_t>( cy0 - 1 ) * cw + cx0 - 4 ) : 0x81818181u;
        else v = load_recon_u32( Cp + static_cast<size_t>( cy0 - 1 ) * cw + cx0 + ( l - 1 ) * 4 );
        *reinterpret_cast<uint32_t *>( &S.L.c[pl][0][l * 4] ) = v;
      } else {
        reinterpret_cast<uint32_t *>( S.bm )[b - 12] = 0;
        if ( b == 12 ) S.trial_mask = 0;
      }
      S.L.y[b + 1][3] = x0 > 0 ? static_cast<uint8_t>( load_recon_u32( Y + static_cast<size_t>( y0 + b ) * pw + x0 - 4 ) >> 24 ) : 129;
      {
        const int pl = b >> 3, r = b & 7, cx0 = col * 8, cy0 = row * 8;
        const uint8_t * Cp = J.recon[1 + pl];
        S.L.c[pl][r + 1][3] = cx0 > 0 ? static_cast<uint8_t>( load_recon_u32( Cp + static_cast<size_t>( cy0 + r ) * cw + cx0 - 4 ) >> 24 ) : 129;
      }
    } );
    lanes.sync();
  }

  // ---- the second pass: the context of a block's first token = how many of the blocks above and to the left of it hold a coefficient
  // (Block::context; beyond the frame: none).  own: the macroblock's own blocks as far as they are settled. ----
  AA_MHD uint32_t y_context( const int b, const uint32_t own ) const
  {
    const uint32_t a = b >= 4 ? ( own >> ( b - 4 ) ) & 1u : ( above_mask >> ( 12 + b ) ) & 1u;
    const uint32_t l = ( b & 3 ) ? ( own >> ( b - 1 ) ) & 1u : ( left_mask >> ( b + 3 ) ) & 1u;
    return a + l;
  }
  // k: 0..7 = plane * 4 + block; own: bit k
  AA_MHD uint32_t uv_context( const int k, const uint32_t own ) const
  {
    const int cb = k & 3;
    const uint32_t a = cb >= 2 ? ( own >> ( k - 2 ) ) & 1u : ( above_mask >> ( 16 + k + 2 ) ) & 1u;
    const uint32_t l = ( cb & 1 ) ? ( own >> ( k - 1 ) ) & 1u : ( left_mask >> ( 16 + k + 1 ) ) & 1u;
    return a + l;
  }
  // What the lanes' blocks leave under each context is known (m0, m1, m2: bit k = block k holds a coefficient under context 0, 1, 2):
  // the blocks in their order, each under the context its settled neighbours give it -> the settled blocks; ctx: block `mine`'s
  template <class F>
  AA_MHD static uint32_t settle( const int blocks, const uint32_t m0, const uint32_t m1, const uint32_t m2, const int mine, uint32_t & ctx, F context )
  {
    uint32_t own = 0;
    ctx = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int k = 0; k < 16; k++ ) {
      if ( k >= blocks ) continue;
      const uint32_t c = context( k, own );
      own |= ( ( ( c == 0 ? m0 : ( c == 1 ? m1 : m2 ) ) >> k ) & 1u ) << k;
      ctx = k == mine ? c : ctx;
    }
    return own;
  }
  // the lane's trellis is built: bit `at` + 8 * ctx of the result = what its walk leaves under that context
  template <class Regs>
  AA_MHD uint32_t outcomes( const Regs & R, const int type, const int at ) const
  {
    const TrellisCosts & T = *C.trellis;
    const bool from0 = R.tr.nonzero_from( 0 ), from1 = R.tr.nonzero_from( 1 );
    uint32_t v = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( uint32_t ctx = 0; ctx < 3; ctx++ ) v |= ( ( R.tr.pick( ctx, type, T, P::rate_mul( C ), P::dist_mul( C ) ) ? from1 : from0 ) ? 1u : 0u ) << ( at + 8 * ctx );
    return v;
  }
  AA_MHD void note_walk( const TrellisTrace & trace ) const { if ( trace.ran && trace.chose_lower ) P::note( C, K2_TRELLIS_NOT_TRUNCATED ); }

  // ---- predictions of lane b's units ----
  AA_MHD void predict16( const int mode, const int b, int ( &p )[16] ) const
  {
    const int bx = ( b & 3 ) * 4, by = ( b >> 2 ) * 4;
    int sa = 0, sl = 0;
    for ( int i = 0; i < 16; i++ ) { sa += S.L.y[0][i + 4]; sl += S.L.y[i + 1][3]; }
    const int dc = bigpred_dc( sa, sl, row > 0, col > 0, 4 ), corner = S.L.y[0][3];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int i = 0; i < 16; i++ ) p[i] = bigpred_pixel( mode, S.L.y[0][bx + ( i & 3 ) + 4], S.L.y[by + ( i >> 2 ) + 1][3], corner, dc );
  }
  AA_MHD void predict_chroma( const int mode, const int pl, const int cb, int ( &p )[16] ) const
  {
    int sa = 0, sl = 0;
    for ( int i = 0; i < 8; i++ ) { sa += S.L.c[pl][0][i + 4]; sl += S.L.c[pl][i + 1][3]; }
    const int dc = bigpred_dc( sa, sl, row > 0, col > 0, 3 ), corner = S.L.c[pl][0][3];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int i = 0; i < 16; i++ ) p[i] = bigpred_pixel( mode, S.L.c[pl][0][( cb & 1 ) * 4 + ( i & 3 ) + 4], S.L.c[pl][( cb >> 1 ) * 4 + ( i >> 2 ) + 1][3], corner, dc );
  }
  AA_MHD void predict_inter( const int b, const int mvx, const int mvy, int ( &p )[16] ) const
  {
    predict_unit( J.ref[1][0], rw(), rh(), tx() + ( b & 3 ) * 4, ty() + ( b >> 2 ) * 4, mvx, mvy, p );
  }
  // the estimate's reconstruction of an inter macroblock predicts again, at the SMALL frame's position of the same reference
  // (reconstruct_inter: raster.Y.inter_predict, macroblock.cc:589-591): that is what later intra neighbours see
  AA_MHD void predict_inter_small( const int b, const int mvx, const int mvy, int ( &p )[16] ) const
  {
    predict_unit( J.ref[1][0], rw(), rh(), x0 + ( b & 3 ) * 4, y0 + ( b >> 2 ) * 4, mvx, mvy, p );
  }

  // ---- what reencode_search.hh asks (variance.cc:32-82, the C++ branch) ----
  AA_MHD uint32_t variance_of_partials()
  {
    const int32_t sum = lanes.sumi( []( int, ReencRegs & R ) { return R.s0; } );
    const uint32_t res = lanes.sum( []( int, ReencRegs & R ) { return R.s1; } );
    return static_cast<uint32_t>( res - ( static_cast<int64_t>( sum ) * sum ) / 256 );
  }
  AA_MHD static void partials( ReencRegs & R, const int ( &p )[16] )
  {
    int s = 0; uint32_t e = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int i = 0; i < 16; i++ ) { const int d = static_cast<int16_t>( R.t[i] - p[i] ); s += d; e += static_cast<uint32_t>( d * d ); }
    R.s0 = s; R.s1 = e;
  }
  AA_MHD uint32_t intra_variance( const int mode )
  {
    lanes.each( [&]( const int b, ReencRegs & R ) { int p[16]; predict16( mode, b, p ); partials( R, p ); } );
    return variance_of_partials();
  }
  AA_MHD uint32_t inter_variance( const int mvx, const int mvy )
  {
    lanes.each( [&]( const int b, ReencRegs & R ) { int p[16]; predict_inter( b, mvx, mvy, p ); partials( R, p ); } );
    return variance_of_partials();
  }
  AA_MHD uint32_t inter_sad( const int mvx, const int mvy )
  {
    return lanes.sum( [&]( const int b, ReencRegs & R ) {
      int p[16];
      predict_inter( b, mvx, mvy, p );
      uint32_t s = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
      for ( int i = 0; i < 16; i++ ) s += static_cast<uint32_t>( iabs( R.t[i] - p[i] ) );
      return s; } );
  }

  // The B_PRED trial (encode_intra.cc:111-141,48-71,360-386): sub-block by sub-block in raster order; a lane is a PIXEL of the
  // sub-block while its mode is chosen, then lane 0 runs the forward path and puts the reconstruction into the slot's picture.
  // The coefficients go straight to the sub-block's slot: whichever mode wins writes every slot it owns afterwards.
  AA_MHD void bpred_trial( uint32_t & rate, uint32_t & distortion )
  {
    for ( int sb = 0; sb < 16; sb++ ) {
      const int bx = sb & 3, by = sb >> 2;
      const int ar = by * 4, ac = bx * 4 + 3;       // index of (row -1, col -1) of this sub-block in the picture
      const uint8_t * target = J.target[0] + static_cast<int64_t>( ty() + by * 4 ) * J.target_stride[0] + tx() + bx * 4;
      lanes.each( [&]( const int b, ReencRegs & R ) {
        if ( b < 13 ) {
          uint8_t e;
          if ( b < 4 ) e = S.L.y[ar + 4 - b][ac];
          else if ( b < 9 ) e = S.L.y[ar][ac + b - 4];
          else e = bx == 3 ? S.L.y[0][20 + b - 9] : S.L.y[ar][ac + b - 4];   // above-right of the fourth column: the row above the MACROBLOCK (prediction.cc:140-164)
          S.L.edge[b] = e;
        }
        R.s0 = target[( b >> 2 ) * J.target_stride[0] + ( b & 3 )];
      } );
      lanes.sync();
      uint32_t sse[10];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
      for ( int m = 0; m < 10; m++ )
        sse[m] = lanes.sum( [&]( const int b, ReencRegs & R ) { const int d = static_cast<int16_t>( R.s0 - bpred_pixel( m, S.L.edge, b & 3, b >> 2 ) ); return static_cast<uint32_t>( d * d ); } );
      const int above_mode = sb >= 4 ? S.bm[sb - 4] : ( row > 0 ? static_cast<int>( ( above.bm_bottom >> ( 8 * sb ) ) & 0xFFu ) : 0 );
      const int left_mode = ( sb & 3 ) ? S.bm[sb - 1] : ( col > 0 ? static_cast<int>( ( left.bm_right >> ( 8 * ( sb >> 2 ) ) ) & 0xFFu ) : 0 );
      const uint16_t * mode_costs = P::bmode( C, above_mode, left_mode );
      uint32_t best_sse = 0;
      const int mode = pick_bmode<P>( C, mode_costs, sse, best_sse );
      rate += mode_costs[mode];
      distortion += best_sse;
      lanes.sync();                                  // (every lane has read bm[] before lane 0 writes it)
      lanes.each( [&]( const int b, ReencRegs & ) {
        S.L.pred[b] = static_cast<uint8_t>( bpred_pixel( mode, S.L.edge, b & 3, b >> 2 ) );
        if ( b == 0 ) S.bm[sb] = static_cast<uint8_t>( mode );
      } );
      lanes.sync();
      lanes.each( [&]( const int b, ReencRegs & ) {
        if ( b != 0 ) return;
        int p[16], q[16];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
        for ( int i = 0; i < 16; i++ ) p[i] = S.L.pred[i];
        forward_block( target, J.target_stride[0], p, q );
        if constexpr ( P::kSecondPass ) {
          // the block's type is the one the FIRST pass ended with (reencode_search.hh): after a 16x16 mode the unquantised DC stays
          const int type = ( C.first_pass[mi] & 1u ) ? TQ_Y_WITHOUT_Y2 : TQ_Y_AFTER_Y2;
          TrellisTrace trace;
          if ( trellis_quantize( q, type, J.quant[Q_Y_DC], J.quant[Q_Y_AC], y_context( sb, S.trial_mask ), *C.trellis, P::rate_mul( C ), P::dist_mul( C ), &trace ) ) S.trial_mask |= 1u << sb;
          note_walk( trace );
        } else {
          if ( quantize_block( q, J.quant[Q_Y_DC], J.quant[Q_Y_AC] ) ) S.trial_mask |= 1u << sb;
        }
        store_block( J.coeffs + ( mi * 25 + sb ) * 16, q );
        uint32_t rows[4];
        reconstruct_block( q, J.quant[Q_Y_DC], J.quant[Q_Y_AC], false, 0, p, rows );
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
        for ( int r = 0; r < 4; r++ ) *reinterpret_cast<uint32_t *>( &S.L.y[ar + r + 1][bx * 4 + 4] ) = rows[r];
      } );
      lanes.sync();
    }
  }

  // ---- the chosen mode applied (encode_intra.cc:169-222, encode_inter.cc:375-435, FIRST_PASS; the statements of k_rebase_*) ----
  // every lane's prediction is in its R.p: 16 luma slots, the Y2 slot, the reconstruction -> mask bits 0..15 and 24
  // (inter, mv: read by the estimate alone, which reconstructs an inter macroblock from another prediction than it coded)
  AA_MHD uint32_t code_luma_with_y2( const bool inter, const Mv mv )
  {
    lanes.each( [&]( const int b, ReencRegs & R ) {
      const int bx = ( b & 3 ) * 4, by = ( b >> 2 ) * 4;
      forward_block( J.target[0] + static_cast<int64_t>( ty() + by ) * J.target_stride[0] + tx() + bx, J.target_stride[0], R.p, R.q );
      S.L.dcs[b] = static_cast<int16_t>( R.q[0] );
      R.q[0] = 0;
      R.nz = quantize_block( R.q, J.quant[Q_Y_DC], J.quant[Q_Y_AC] );
      store_block( J.coeffs + ( mi * 25 + b ) * 16, R.q );
    } );
    lanes.sync();
    lanes.each( [&]( const int b, ReencRegs & R ) {
      const int bx = ( b & 3 ) * 4, by = ( b >> 2 ) * 4;
      int q2[16], dc_back;
      R.nz2 = y2_block( S.L.dcs, J.quant, b, q2, dc_back );
      if ( b == 0 ) store_block( J.coeffs + ( mi * 25 + 24 ) * 16, q2 );
      if constexpr ( P::kSampled ) { if ( inter ) predict_inter_small( b, mv.x, mv.y, R.p ); }
      uint32_t rows[4];
      reconstruct_block( R.q, J.quant[Q_Y_DC], J.quant[Q_Y_AC], true, dc_back, R.p, rows );
      store_rows( J.recon[0] + static_cast<size_t>( y0 + by ) * pw + x0 + bx, pw, rows );
    } );
    lanes.sync();                                    // (dcs[] is read before the next macroblock of this slot writes it)
    return lanes.sum( []( const int b, ReencRegs & R ) { return ( R.nz ? 1u << b : 0u ) | ( b == 0 && R.nz2 ? 1u << 24 : 0u ); } );
  }
  // ... in the second pass (luma_mb_apply_intra_prediction under SECOND_PASS): sixteen trellises built at once, their picks settled in
  // block order, check_reset_y2 and the Y2 block's own trellis under the Y2 flags of the macroblocks above and to the left
  AA_MHD uint32_t code_luma_with_y2_second()
  {
    using Regs = typename Lanes::Regs;
    const TrellisCosts & T = *C.trellis;
    const uint32_t rm = P::rate_mul( C ), dm = P::dist_mul( C );
    lanes.each( [&]( const int b, Regs & R ) {
      const int bx = ( b & 3 ) * 4, by = ( b >> 2 ) * 4;
      forward_block( J.target[0] + static_cast<int64_t>( ty() + by ) * J.target_stride[0] + tx() + bx, J.target_stride[0], R.p, R.q );
      S.L.dcs[b] = static_cast<int16_t>( R.q[0] );
      R.q[0] = 0;
      R.tr.build( R.q, TQ_Y_AFTER_Y2, J.quant[Q_Y_DC], J.quant[Q_Y_AC], T, rm, dm );
      const uint32_t o = outcomes( R, TQ_Y_AFTER_Y2, 0 );
      R.s1 = ( ( o & 1u ) << b ) | ( ( ( o >> 8 ) & 1u ) << ( 16 + b ) );
      R.s0 = static_cast<int32_t>( ( ( o >> 16 ) & 1u ) << b );
    } );
    const uint32_t m01 = lanes.sum( []( int, Regs & R ) { return R.s1; } );
    const uint32_t m2 = lanes.sum( []( int, Regs & R ) { return static_cast<uint32_t>( R.s0 ); } );
    lanes.each( [&]( const int b, Regs & R ) {
      uint32_t ctx;
      settle( 16, m01 & 0xFFFFu, m01 >> 16, m2, b, ctx, [&]( const int k, const uint32_t own ) { return y_context( k, own ); } );
      TrellisTrace trace;
      R.nz = R.tr.walk( R.q, R.tr.pick( ctx, TQ_Y_AFTER_Y2, T, rm, dm ), J.quant[Q_Y_DC], J.quant[Q_Y_AC], &trace );
      note_walk( trace );
      store_block( J.coeffs + ( mi * 25 + b ) * 16, R.q );
    } );
    lanes.sync();
    // (above.mv / left.mv: the neighbours' side words of the second pass -- bit 0 the Y2 flag they show, bit 1 B_PRED; see run())
    const uint32_t y2_ctx = ( above.mv & 1u ) + ( left.mv & 1u );
    lanes.each( [&]( const int b, Regs & R ) {
      const int bx = ( b & 3 ) * 4, by = ( b >> 2 ) * 4;
      int q2[16];
      y2_forward( S.L.dcs, q2 );
      bool held = false, holds = false;
      for ( int i = 0; i < 16; i++ ) held |= q2[i] != 0;
      check_reset_y2( q2, J.quant[Q_Y2_DC], J.quant[Q_Y2_AC] );
      for ( int i = 0; i < 16; i++ ) holds |= q2[i] != 0;
      TrellisTrace trace;
      R.nz2 = trellis_quantize( q2, TQ_Y2, J.quant[Q_Y2_DC], J.quant[Q_Y2_AC], y2_ctx, T, rm, dm, &trace );
      if ( b == 0 ) {
        note_walk( trace );
        if ( held && !holds ) P::note( C, K2_Y2_RESET );
        if ( trace.ran && ( ( above.mv & 2u ) || ( left.mv & 2u ) ) ) P::note( C, K2_STALE_Y2_CONTEXT );
        if ( trace.ran && ( ( above.mv & 3u ) == 3u || ( left.mv & 3u ) == 3u ) ) P::note( C, K2_STALE_Y2_SET );
        store_block( J.coeffs + ( mi * 25 + 24 ) * 16, q2 );
      }
      uint32_t rows[4];
      reconstruct_block( R.q, J.quant[Q_Y_DC], J.quant[Q_Y_AC], true, y2_back( q2, J.quant, b ), R.p, rows );
      store_rows( J.recon[0] + static_cast<size_t>( y0 + by ) * pw + x0 + bx, pw, rows );
    } );
    lanes.sync();                                    // (dcs[] is read before the next macroblock of this slot writes it)
    return lanes.sum( []( const int b, Regs & R ) { return ( R.nz ? 1u << b : 0u ) | ( b == 0 && R.nz2 ? 1u << 24 : 0u ); } );
  }
  // ... and the chroma blocks of the chosen mode (chroma_mb_apply_intra_prediction under SECOND_PASS): lanes 0..7 one block each, U's
  // and V's picks settled plane by plane -> mask bits 16..23
  AA_MHD uint32_t code_chroma_second( const int mode )
  {
    using Regs = typename Lanes::Regs;
    const TrellisCosts & T = *C.trellis;
    const uint32_t rm = P::rate_mul( C ), dm = P::dist_mul( C );
    const uint32_t m = lanes.sum( [&]( const int b, Regs & R ) {
      if ( b >= 8 ) return 0u;
      const int pl = b >> 2, cb = b & 3;
      predict_chroma( mode, pl, cb, R.p );
      forward_block( J.target[1 + pl] + static_cast<int64_t>( tcy() + ( cb >> 1 ) * 4 ) * J.target_stride[1] + tcx() + ( cb & 1 ) * 4, J.target_stride[1], R.p, R.q );
      R.tr.build( R.q, TQ_UV, J.quant[Q_UV_DC], J.quant[Q_UV_AC], T, rm, dm );
      return outcomes( R, TQ_UV, b ); } );
    return lanes.sum( [&]( const int b, Regs & R ) {
      if ( b >= 8 ) return 0u;
      const int pl = b >> 2, cb = b & 3;
      uint32_t ctx;
      settle( 8, m & 0xFFu, ( m >> 8 ) & 0xFFu, ( m >> 16 ) & 0xFFu, b, ctx, [&]( const int k, const uint32_t own ) { return uv_context( k, own ); } );
      TrellisTrace trace;
      const bool nz = R.tr.walk( R.q, R.tr.pick( ctx, TQ_UV, T, rm, dm ), J.quant[Q_UV_DC], J.quant[Q_UV_AC], &trace );
      note_walk( trace );
      store_block( J.coeffs + ( mi * 25 + 16 + b ) * 16, R.q );
      uint32_t rows[4];
      reconstruct_block( R.q, J.quant[Q_UV_DC], J.quant[Q_UV_AC], false, 0, R.p, rows );
      store_rows( J.recon[1 + pl] + static_cast<size_t>( row * 8 + ( cb >> 1 ) * 4 ) * cw + col * 8 + ( cb & 1 ) * 4, cw, rows );
      return nz ? 1u << ( 16 + b ) : 0u; } );
  }

  // B_PRED won: its coefficients are in their slots, its reconstruction is in the picture
  AA_MHD uint32_t keep_bpred()
  {
    lanes.each( [&]( const int b, ReencRegs & ) {
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
      for ( int c4 = 0; c4 < 16; c4 += 4 )
        *reinterpret_cast<uint32_t *>( J.recon[0] + static_cast<size_t>( y0 + b ) * pw + x0 + c4 ) = *reinterpret_cast<const uint32_t *>( &S.L.y[b + 1][c4 + 4] );
    } );
    return S.trial_mask;
  }
  // chroma_block (rebase_inl.hh) for the estimate: the original read at the original's position, the prediction that is coded (p) and the
  // one the reconstruction is made from (ps: the same but for an inter macroblock), the reconstruction at the small frame's position
  AA_MHD bool chroma_block_sampled( const int pl, const int cb, const int ( &p )[16], const int ( &ps )[16] )
  {
    const int bx = ( cb & 1 ) * 4, by = ( cb >> 1 ) * 4;
    int q[16];
    forward_block( J.target[1 + pl] + static_cast<int64_t>( tcy() + by ) * J.target_stride[1] + tcx() + bx, J.target_stride[1], p, q );
    const bool nz = quantize_block( q, J.quant[Q_UV_DC], J.quant[Q_UV_AC] );
    store_block( J.coeffs + ( mi * 25 + 16 + pl * 4 + cb ) * 16, q );
    uint32_t rows[4];
    reconstruct_block( q, J.quant[Q_UV_DC], J.quant[Q_UV_AC], false, 0, ps, rows );
    store_rows( J.recon[1 + pl] + static_cast<size_t>( row * 8 + by ) * cw + col * 8 + bx, cw, rows );
    return nz;
  }

  // chroma of an intra macroblock: uv_mode by distortion alone (pick_uv_mode), then lanes 0..7 one block each -> mask bits 16..23
  AA_MHD uint32_t code_chroma_intra( int & uv_mode )
  {
    uint32_t sse[4];
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
    for ( int m = 0; m < 4; m++ )
      sse[m] = lanes.sum( [&]( const int b, ReencRegs & ) {
        if ( b >= 8 ) return 0u;
        const int pl = b >> 2, cb = b & 3;
        int p[16];
        predict_chroma( m, pl, cb, p );
        const uint8_t * t = J.target[1 + pl] + static_cast<int64_t>( tcy() + ( cb >> 1 ) * 4 ) * J.target_stride[1] + tcx() + ( cb & 1 ) * 4;
        uint32_t e = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
#pragma unroll
#endif
        for ( int i = 0; i < 16; i++ ) { const int d = static_cast<int16_t>( t[( i >> 2 ) * J.target_stride[1] + ( i & 3 )] - p[i] ); e += static_cast<uint32_t>( d * d ); }
        return e; } );
    const int mode = pick_uv_mode( sse );
    uv_mode = mode;
    if constexpr ( P::kSecondPass ) return code_chroma_second( mode );
    else return lanes.sum( [&]( const int b, ReencRegs & ) {
      if ( b >= 8 ) return 0u;
      int p[16];
      predict_chroma( mode, b >> 2, b & 3, p );
      if constexpr ( P::kSampled ) return chroma_block_sampled( b >> 2, b & 3, p, p ) ? 1u << ( 16 + b ) : 0u;
      else return chroma_block( J, mi, col, row, b >> 2, b & 3, p ) ? 1u << ( 16 + b ) : 0u; } );
  }
  // chroma of an inter macroblock: the rounded average of four equal luma vectors (chroma_mb_inter_predict)
  AA_MHD uint32_t code_chroma_inter( const int mvx, const int mvy )
  {
    const int cx = chroma_mv( 4 * mvx ), cy = chroma_mv( 4 * mvy );
    return lanes.sum( [&]( const int b, ReencRegs & ) {
      if ( b >= 8 ) return 0u;
      const int pl = b >> 2, cb = b & 3;
      int p[16];
      if constexpr ( P::kSampled ) {
        int ps[16];
        predict_unit( J.ref[1][1 + pl], rw() / 2, rh() / 2, tcx() + ( cb & 1 ) * 4, tcy() + ( cb >> 1 ) * 4, cx, cy, p );
        predict_unit( J.ref[1][1 + pl], rw() / 2, rh() / 2, col * 8 + ( cb & 1 ) * 4, row * 8 + ( cb >> 1 ) * 4, cx, cy, ps );
        return chroma_block_sampled( pl, cb, p, ps ) ? 1u << ( 16 + b ) : 0u;
      } else {
        predict_unit( J.ref[1][1 + pl], cw, ch, col * 8 + ( cb & 1 ) * 4, row * 8 + ( cb >> 1 ) * 4, cx, cy, p );
        return chroma_block( J, mi, col, row, pl, cb, p ) ? 1u << ( 16 + b ) : 0u;
      } } );
  }

  // The macroblock: census, decision, the chosen mode applied, its record and its side record.
  AA_MHD void run()
  {
    stage();
    const unsigned mbw = J.mbw, mbh = J.mbh;
    ReencNeighbour above_left;
    above.inter = left.inter = above_left.inter = 0;
    above.mv = left.mv = above_left.mv = 0; above_left.bm_bottom = above_left.bm_right = 0; above.bm_bottom = above.bm_right = left.bm_bottom = left.bm_right = 0;
    if ( row > 0 ) above = neighbour( mi - mbw );
    if ( col > 0 ) left = neighbour( mi - 1 );
    if constexpr ( !P::kKey ) { if ( row > 0 && col > 0 ) above_left = neighbour( mi - mbw - 1 ); }      // (a key frame takes no census)
    if constexpr ( P::kSecondPass ) {
      if ( row > 0 ) above_mask = load_recon_u32( reinterpret_cast<const uint8_t *>( J.masks + mi - mbw ) );
      if ( col > 0 ) left_mask = load_recon_u32( reinterpret_cast<const uint8_t *>( J.masks + mi - 1 ) );
    }
    const ReencCensus cen = [&]() {
      if constexpr ( P::kKey ) return ReencCensus();
      else return census( above, left, above_left, P::inter( C ).mv_counts_to_probs, static_cast<unsigned>( col ), static_cast<unsigned>( row ), mbw, mbh );
    }();
    const ReencChoice choice = choose_prediction<P>( *this, C, cen, static_cast<unsigned>( col ), static_cast<unsigned>( row ), mbw, mbh );
    const int mode = choice.mode;
    const bool inter = !P::kKey && mode > B_PRED;
    uint32_t mask;
    int uv_mode = 0;
    if ( mode == B_PRED ) mask = keep_bpred();
    else {
      lanes.each( [&]( const int b, ReencRegs & R ) {
        if constexpr ( P::kKey ) predict16( mode, b, R.p );
        else { if ( inter ) predict_inter( b, choice.mv.x, choice.mv.y, R.p ); else predict16( mode, b, R.p ); } } );
      if constexpr ( P::kSecondPass ) mask = code_luma_with_y2_second();
      else mask = code_luma_with_y2( inter, choice.mv );
    }
    // the second pass's side word (a key frame has no vector): bit 0 = the Y2 flag the macroblocks to the right and below see -- this
    // pass's where a Y2 block is coded, the first pass's where B_PRED leaves the block alone -- and bit 1 = B_PRED
    uint32_t side_word = 0;
    if constexpr ( P::kSecondPass ) {
      side_word = mode == B_PRED ? ( ( C.first_pass[mi] >> 1 ) & 1u ) | 2u : ( mask >> 24 ) & 1u;
      if ( mode == B_PRED && !( C.first_pass[mi] & 1u ) ) P::note( C, K2_BPRED_AFTER_16X16 );
    }
    if constexpr ( !P::kKey ) mask |= inter ? code_chroma_inter( choice.mv.x, choice.mv.y ) : code_chroma_intra( uv_mode );
    else mask |= code_chroma_intra( uv_mode );

    // the record (what the parser would say of the serialised macroblock, but for flags, coeff_index and lf_level: the host's) and
    // the side record for the macroblocks to the right and below
    constexpr uint32_t kImplied[4] = { B_DC_PRED, B_VE_PRED, B_HE_PRED, B_TM_PRED };        // macroblock.hh:134-143
    const uint32_t implied = ( mode == V_PRED ? kImplied[1] : ( mode == H_PRED ? kImplied[2] : ( mode == TM_PRED ? kImplied[3] : kImplied[0] ) ) ) * 0x01010101u;
    const uint32_t mvw = ( static_cast<uint32_t>( static_cast<uint16_t>( choice.mv.x ) ) ) | ( static_cast<uint32_t>( static_cast<uint16_t>( choice.mv.y ) ) << 16 );
    lanes.each( [&]( const int b, ReencRegs & ) {
      uint32_t * rec = reinterpret_cast<uint32_t *>( RJ.mbs_out + mi );
      const uint32_t bmw = b < 4 ? ( mode < B_PRED ? implied : reinterpret_cast<const uint32_t *>( S.bm )[b] ) : 0u;
      rec[4 + b] = inter ? mvw : bmw;
      if ( b == 0 ) {
        rec[0] = static_cast<uint32_t>( mode ) | ( static_cast<uint32_t>( uv_mode ) << 8 ) | ( inter ? 1u << 16 : 0u );
        rec[1] = 0; rec[2] = mask; rec[3] = 0;
        J.masks[mi] = mask;
        uint32_t * nb = RJ.nb + mi * 4;
        if constexpr ( P::kSecondPass ) nb[0] = side_word; else nb[0] = mvw;
        nb[1] = inter ? 1u : 0u;
        if ( mode < B_PRED ) { nb[2] = implied; nb[3] = implied; }
        else {
          nb[2] = reinterpret_cast<const uint32_t *>( S.bm )[3];
          nb[3] = static_cast<uint32_t>( S.bm[3] ) | ( static_cast<uint32_t>( S.bm[7] ) << 8 ) | ( static_cast<uint32_t>( S.bm[11] ) << 16 ) | ( static_cast<uint32_t>( S.bm[15] ) << 24 );
        }
      }
    } );
    lanes.sync();
  }
};

} // namespace
} // namespace aa
