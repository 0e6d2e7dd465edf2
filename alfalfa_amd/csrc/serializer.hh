// Host half of the serialisation (aa_serialize_batch): records -> the frame header and first partition, and the frame put together.
//
// Restates, from the algorithm and over the RECORDS (aa_frame_header + aa_frame_header_ext + aa_mb_info), what the reference does in
//   encode( KeyFrameHeader / InterFrameHeader ) (serializer.cc:110-181, frame_header.hh:194-295),
//   Macroblock::serialize + encode_prediction_modes (serializer.cc:187-385): segment id, skip flag, reference, modes, motion vectors
//   against the census (the same census parse_common.hh restates for the parse), ProbabilityTables::update (the frame's own tables),
//   make_frame (serializer.cc:741-799).
// The DCT partitions are serialize_common.hh's: on the device in the product, on the host in serialize_frame_host (tests, tools).
#pragma once
#include <cstdint>
#include <vector>

#include "parser.hh"

namespace aa {

// The tables a frame is coded with: `before` (1101 bytes as aa_parser_get_probs lays them out; a key frame starts from the defaults
// instead) with the header's token, mode and motion-vector updates applied (ProbabilityTables::coeff_prob_update / update).
void frame_probs( const uint8_t * before, bool key_frame, const aa_frame_header_ext & x, ProbTables & out );

// Frame::serialize_first_partition: the frame header, then every macroblock's header, then BoolEncoder::finish.
// Throws ParseError( AA_ERR_ARGUMENT ) on records no bitstream can say (a mode out of range, an inter macroblock in a key frame).
// sub_modes (may be null): the sub-block modes of the SPLITMV macroblocks' partitions in bitstream order, as Parser::last_sub_modes gives
// them for the frame the records came from (a rebased frame: for its prediction frame).  A record holds a partition's vector, not the mode
// that said it; where a listed mode gives the record's vector it is written, else -- and for every partition beyond the list -- the first
// of LEFT4X4, ABOVE4X4, ZERO4X4 that gives the vector, NEW4X4 otherwise.  Every choice parses back to the same records.
void write_first_partition( const aa_frame_header & h, const aa_frame_header_ext & x, const ProbTables & t, const aa_mb_info * mbs, const uint8_t * sub_modes, size_t n_sub_modes,
                            std::vector<uint8_t> & out );

// make_frame: tag, key-frame start code and size, first partition, partition lengths, partitions.  -> the frame's size; written only if
// it fits `capacity`.
size_t assemble_frame( const aa_frame_header & h, const std::vector<uint8_t> & first, const uint8_t * const * parts, const uint32_t * sizes, uint8_t * out, size_t capacity );

// The whole frame on the host: coeffs = dense blocks, a macroblock's at coeff_index (what aa_parser_parse / aa_stream_read_records return).
void serialize_frame_host( const aa_frame_header & h, const aa_frame_header_ext & x, const uint8_t * probs_before, const aa_mb_info * mbs, const int16_t * coeffs,
                           const uint8_t * sub_modes, size_t n_sub_modes, std::vector<uint8_t> & out );

// The bytes of an estimate's frame (Encoder::estimate_size, size_estimation.cc): the small frame of small_w x small_h pixels (the
// original's size / 4, truncated) under a header as the reference's persistent subsampled frame has it -- everything default but y_ac_qi,
// refresh_entropy_probs, an inter frame's refresh_last, prob_skip_false (optimize_prob_skip: always set) and, an inter frame, the three
// reference probabilities (optimize_interframe_probs: each only where its new value is above zero, else what the estimate before left:
// carry[0..2], in and out; a key estimate neither reads nor writes it) -- no token probability update, one DCT partition.  recs / masks: what
// the decision left (y_mode, uv_mode, ref_frame, u; raw masks); token_bytes, with_coefficients, intra: est::write_tokens' counts;
// probs_before: the tables before the frame (1101 bytes; a key estimate starts from the defaults and may pass null).
// -> tag + first partition + the DCT partition.  The estimate is sixteen times this.
size_t estimate_frame_bytes( bool key_frame, uint16_t small_w, uint16_t small_h, uint8_t q_index, const uint8_t * probs_before, const aa_mb_info * recs, const uint32_t * masks,
                             uint32_t token_bytes, uint32_t with_coefficients, uint32_t intra, uint8_t carry[4] );

} // namespace aa
