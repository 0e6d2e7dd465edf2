// runtime.cpp (ABI): the forward encoder (aa_encode_batch / aa_encode_device_batch; Encoder::encode_with_quantizer, encoder.cc:559-575) --
// rasters in device memory encoded as key frames (encode_raster<KeyFrame>) or as inter frames predicted from the job streams' current last
// references (encode_raster<InterFrame>), first pass, the header the caller's.  The job checks, the slicing, the cost-block upload, the
// records, the compaction, the append and the timing are the re-encode's two entries (runtime_reencode.inc), instantiated for this caller:
// what differs -- key jobs, the forward cost blocks, a kernel per kind (encode_kernels.hip) -- stands there behind Call::kForward.
// aa_encode_two_pass_batch / aa_encode_two_pass_device_batch: the same calls with, per job, the flag that a KEY job runs the reference's
// second pass (encode_intra.cc:409-439) behind its first -- k_key2_first_pass, k_key2_updates, k_encode_key2 -- and the first pass's
// token_prob_update beside the result (TwoPassArgs, runtime_reencode.inc).
namespace {

struct EncodeCall {
  static constexpr bool kForward = true;
  static constexpr const char * kHost = "aa_encode_batch", * kDevice = "aa_encode_device_batch";
  static double * timing( aa_ctx * ctx ) { return ctx->encode_timing; }
};

} // namespace

extern "C" {

aa_status aa_encode_batch( aa_ctx * ctx, aa_encode_job * jobs, int n ) { return reencode_batch<EncodeCall>( ctx, jobs, n ); }
aa_status aa_encode_device_batch( aa_ctx * ctx, aa_encode_device_job * jobs, int n ) { return reencode_device_batch<EncodeCall>( ctx, jobs, n ); }

aa_status aa_encode_two_pass_batch( aa_ctx * ctx, aa_encode_job * jobs, int n, const uint8_t * two_pass, uint8_t * first_pass_updates )
{
  if ( !two_pass || !first_pass_updates ) return fail( AA_ERR_ARGUMENT, "aa_encode_two_pass_batch: null argument" );
  TwoPassArgs tp; tp.flags = two_pass; tp.updates = first_pass_updates;
  return reencode_batch<EncodeCall>( ctx, jobs, n, tp );
}
aa_status aa_encode_two_pass_device_batch( aa_ctx * ctx, aa_encode_device_job * jobs, int n, const uint8_t * two_pass, uint8_t * first_pass_updates )
{
  if ( !two_pass || !first_pass_updates ) return fail( AA_ERR_ARGUMENT, "aa_encode_two_pass_device_batch: null argument" );
  TwoPassArgs tp; tp.flags = two_pass; tp.updates = first_pass_updates;
  return reencode_device_batch<EncodeCall>( ctx, jobs, n, tp );
}

aa_status aa_encode_last_timing( aa_ctx * ctx, double out[5] )
{
  if ( !ctx || !out ) return fail( AA_ERR_ARGUMENT, "aa_encode_last_timing: null argument" );
  std::memcpy( out, ctx->encode_timing, sizeof ctx->encode_timing );
  return AA_OK;
}

} // extern "C"
