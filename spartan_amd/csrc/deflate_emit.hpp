// spartan_amd: what deflate_match.hip needs of the device coder (deflate_emit.hip) to queue it behind its parse kernels.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

struct DeEmit;
// tokens an open block carries from one segment's list to the next: tdefl::BLOCK_TOKENS rounded up to whole workgroups
constexpr uint32_t DE_CARRY = 58368;
constexpr size_t DE_REC_WORDS = 6, DE_HIST = 320, DE_HDR_BYTES = 320, DE_PLAN_WORDS = 6;
// blocks a list of `tokens` tokens can close: a block that is not the last holds more than 11306 tokens (its code buffer is fuller than
// 31744 * 128 / 115 bytes at three bytes and an eighth a token); one more for the finish block, one for rounding
inline size_t de_max_blocks(size_t tokens) { return tokens / 11306 + 2; }

int32_t de_open(DeEmit** out, hipStream_t st, const uint8_t* dD, size_t n, size_t seg, size_t nseg, size_t chunk);
void de_close(DeEmit* e);
uint32_t* de_tokens(DeEmit* e, size_t s);  // device: where segment s's compacted tokens go (seg + 1 words)
size_t* de_ntok(DeEmit* e, size_t s);      // device: their number
// queue segment s's block stage behind its compaction: the open block's tokens carried in, costs, scan, boundaries, histograms, Adler-32, and
// the copy of the records into pinned slot s & 1
int32_t de_segment_blocks(DeEmit* e, size_t s, size_t first, size_t count);
// after that copy has arrived: the segment's closed blocks, laid out as spz_deflate_blocks_host's; valid until segment s + 2 is queued
int32_t de_blocks(DeEmit* e, size_t s, size_t* nblocks, const uint64_t** records, const uint16_t** hist, uint64_t adler[2]);
int32_t de_segment_emit(DeEmit* e, size_t s, size_t nblocks, const uint64_t* plans, const uint32_t* tables, const uint8_t* hdrs);
int32_t de_bytes(DeEmit* e, uint8_t* out, size_t nbytes, double* ms);
