/* spartan_host.h: the C boundary of the host driver (libspartan_host.so; spartan_amd/host/host_capi.cc), which mirrors libspartan's
 * SNARK / NIZK API on top of the device library's C ABI (spartan_hip.h). This header is the one declaration of every spz_* entry point:
 * host_capi.cc is compiled against it with -Wmissing-prototypes as an error, spartan_amd/prover.py binds from a table that
 * tests/test_host_abi.py compares with it, and the same test checks the hand-written Rust declarations of rust_shim/src/gpu_tail.rs.in.
 *
 * Conventions. Handles are void*: what a *_new / *_load / *_encode / *_prove entry returned, given back to the matching *_free exactly
 * once. Scalars cross as 4 little-endian 64-bit limbs in Montgomery form unless an entry says "canonical bytes". Nothing throws across
 * the boundary: a failure is a NULL handle or the error code the entry documents, with its text in spz_last_error(). An entry that
 * returns bytes follows one idiom, "size, then fill": it returns the number of bytes and writes them only when out != NULL and
 * cap >= that number, so a first call with (NULL, 0) asks for the size. */
#ifndef SPARTAN_HOST_H
#define SPARTAN_HOST_H

#include "spartan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The text of the last failure on the calling thread. Meaningful ONLY right after a call that reported failure (a NULL handle, a negative
 * code): an entry that can fail clears it on entry, one that cannot fail leaves it alone, so after a success it is empty or stale. The
 * pointer stays valid until the thread's next spz_* call. */
const char* spz_last_error(void);

/* ---- context, options, sharded commitments ---- */
void* spz_ctx_new(int device);
void spz_ctx_free(void* ctx);
sp_ctx* spz_ctx_raw(void* ctx); /* the underlying context of the device library */
/* library options of the context (spartan_hip.h: sp_ctx_set_option, whose code is returned); ctx == NULL: the process-wide defaults */
int spz_ctx_set_option(void* ctx, const char* key, const char* value);
/* which form of Keccak-f[1600] the driver picked for this CPU: "plain", "bmi2" or "avx512" */
const char* spz_keccak_variant(void);

/* The caller's all-gather of a sharded commitment: on entry buf[off, off + len) holds this rank's bytes, on return buf[0, total) is
 * complete. 0 = ok. */
typedef int (*spz_commit_gather_fn)(void* user, uint8_t* buf, size_t total, size_t off, size_t len);
/* Row-sharded commitments across `world` lock-step ranks, the bytes moved by the caller's `gather`; world <= 1 clears the setting
 * (gather may then be NULL). Configuring is itself a collective: every rank calls it at the same point, and gather already works.
 * 0 = ok, -1 = error. */
int spz_ctx_set_commit_shard(void* ctx, int rank, int world, spz_commit_gather_fn gather, void* user);
/* The same with RCCL inside the library: rank 0 draws the id, the caller distributes it, every rank joins. 0 = ok, -1 = error. */
int spz_rccl_unique_id(uint8_t out[128]);
int spz_ctx_set_commit_shard_rccl(void* ctx, int rank, int world, const uint8_t unique_id[128]);
/* nshards shards on one GPU, gathered in-process (the partitioning without a second GPU); nshards <= 1 clears it. 0 = ok, -1 = error. */
int spz_ctx_set_commit_shard_virtual(void* ctx, int nshards);
/* out[0] = exchanges, out[1] = bytes exchanged since the last reset */
void spz_ctx_shard_stats(void* ctx, int reset, uint64_t out[2]);

/* ---- instances ---- */
/* Instance::new (lib.rs:121-228): the entries of A, B, C back to back, nnz[k] of each, as (row, col, 32 canonical little-endian bytes).
 * NULL on failure; an entry is checked for its index first, then for its scalar, and the first failing entry decides:
 * spz_last_error() is "InvalidIndex" or "InvalidScalar", as R1CSError. */
void* spz_instance_new(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], const uint64_t* rows,
                       const uint64_t* cols, const uint8_t* vals);
/* Instance::new on the device: the same arguments and the same two errors, with what the check found. NULL on failure; *status (may be
 * NULL) = SP_OK, SP_EINDEX ("InvalidIndex: ..."), SP_ESCALAR ("InvalidScalar: ...") or SP_EINVAL for anything else; *matrix (may be NULL)
 * = 0, 1, 2 for the matrix that failed, -1 otherwise; report (may be NULL, 4 words) = that matrix's report as sp_sparse_from_entries
 * gives it, (0, UINT64_MAX, 0, UINT64_MAX) on success. */
void* spz_instance_from_entries(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], const uint64_t* rows,
                                const uint64_t* cols, const uint8_t* vals, int32_t* status, int* matrix, uint64_t report[4]);
/* The same from device memory: rows[k], cols[k], vals[k] are the three lists of matrix k in the memory of the context's device, written
 * and complete before the call. */
void* spz_instance_from_device_entries(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3],
                                       const uint64_t* const rows[3], const uint64_t* const cols[3], const uint8_t* const vals[3],
                                       int32_t* status, int* matrix, uint64_t report[4]);
/* Instance::produce_synthetic_r1cs with a seed; the satisfying assignment goes to vars_out (num_vars scalars) and inputs_out (num_inputs
 * scalars), either of which may be NULL. NULL on failure. */
void* spz_instance_synthetic(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, uint64_t seed, uint64_t* vars_out,
                             uint64_t* inputs_out);
void spz_instance_free(void* inst);
/* R1CSShape::get_digest (r1cs.rs:154-158): the zlib stream the proofs absorb, computed on first use (option digest.device: 1 = stream and match
 * search on the device, parser and coding on the calling thread; 2 = the lazy parse on the device too, the calling thread codes its tokens;
 * 3 = the coder on the device too, the calling thread builds each block's Huffman tables and bit offsets; 0 = all of it on the host; the
 * same bytes). Size, then fill; 0 with
 * spz_last_error() when the computation failed (a zlib stream is never empty). */
size_t spz_instance_digest(void* inst, uint8_t* out, size_t cap);
/* A caller that already holds the digest of a real libspartan Instance sets it instead. */
void spz_instance_set_digest(void* inst, const uint8_t* digest, size_t n);
/* zlib header of the COMPUTED digest: 0 = 0x78 0x9C (miniz >= 2.2, miniz_oxide >= 0.4), 1 = 0x78 0x01 (older). An explicit parameter of the
 * instance; call before the digest is first used. 0 = ok, -1 = a digest with the other header has already been computed or set. */
int spz_instance_set_digest_header(void* inst, int old_header);
/* Instance::is_sat (lib.rs:230-259) with the report of the device check: 1 = satisfied, 0 = not, -1 = error ("InvalidNumberOfInputs" as
 * R1CSError). `assignment` (a spz_vars_assignment_* handle) or `vars` (host scalars), the other NULL. report (may be NULL): report[0] =
 * violated constraints, report[1] = the first (UINT64_MAX when none); rows_out (may be NULL) receives the min(report[0], rows_cap)
 * lowest violated constraint numbers. */
int spz_instance_is_sat(void* inst, void* assignment, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                        uint64_t report[2], uint64_t* rows_out, size_t rows_cap);

/* ---- generators ---- */
/* SNARKGens::new / NIZKGens::new: the prover's generators, with fixed-base window tables. NULL on failure. */
void* spz_snark_gens_new(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries);
void* spz_nizk_gens_new(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs);
/* The verifier's generators: the same handle type, taken by every spz_*_verify* entry, by spz_commitment_encode and by
 * spz_snark_gens_stream; refused by spz_snark_encode, every spz_*_prove* and the window-table accessors. NULL on failure. */
void* spz_snark_verifier_gens_new(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries);
void* spz_nizk_verifier_gens_new(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs);
int spz_snark_gens_is_verifier_only(void* gens); /* 1 or 0 */
int spz_nizk_gens_is_verifier_only(void* gens);
size_t spz_snark_gens_resident_bytes(void* gens); /* HBM held by the tables of the handle's streams, either kind */
size_t spz_nizk_gens_resident_bytes(void* gens);
void spz_snark_gens_free(void* gens);
void spz_nizk_gens_free(void* gens);
/* the compressed points of generator stream `which` (0: gens_r1cs_sat, 1: gens_r1cs_eval). Size, then fill. */
size_t spz_snark_gens_stream(void* gens, int which, uint8_t* out, size_t cap);
/* Geometry of the fixed-base window tables of stream `which`: signed window width, windows per scalar, HBM held. A verifier-only handle
 * has no such tables: -1, -1 and 0 with spz_last_error(). */
int spz_snark_gens_window_bits(void* gens, int which);
int spz_snark_gens_windows(void* gens, int which);
size_t spz_snark_gens_table_bytes(void* gens, int which);
/* bincode(SNARKGens). Size, then fill. */
size_t spz_snark_gens_bincode(void* gens, uint8_t* out, size_t cap);

/* ---- SNARK::encode and the verifier's commitment handle ---- */
/* SNARK::encode (lib.rs:325-336): commitment and decommitment in one handle, for spz_snark_prove*. NULL on failure. */
void* spz_snark_encode(void* ctx, void* inst, void* gens);
void spz_encode_free(void* enc);
/* bincode(ComputationCommitment) / bincode(ComputationDecommitment) of an encode handle. Size, then fill; the decommitment downloads its
 * tables and returns 0 with spz_last_error() when that fails. */
size_t spz_commitment_bincode(void* enc, uint8_t* out, size_t cap);
size_t spz_decommitment_bincode(void* enc, uint8_t* out, size_t cap);
/* the share vector `which` (0: comm_comb_ops, 1: comm_comb_mem): returns the number of POINTS, writes 32 bytes each when cap >= 32 * that */
size_t spz_encode_comm(void* enc, int which, uint8_t* out, size_t cap);
/* ComputationCommitment::deserialize of untrusted bytes (what spz_commitment_bincode writes): the verifier's handle of a circuit, with
 * both share vectors uploaded as resident point sets (64 KiB of HBM a share). NULL with spz_last_error() for bytes that are not one
 * commitment, or that hold a share that does not decode. */
void* spz_commitment_load(void* ctx, const uint8_t* bytes, size_t len);
/* The same handle computed from the instance itself: the verifier runs the public preprocessing instead of trusting bytes. `gens` of
 * either kind; under verifier-only generators no window table is ever built. No decommitment is kept. NULL on failure. */
void* spz_commitment_encode(void* ctx, void* inst, void* gens);
/* bincode(ComputationCommitment) of a handle, however it was made. Size, then fill; 0 for a NULL handle. */
size_t spz_commitment_serialize(void* comm, uint8_t* out, size_t cap);
/* HBM held by the handle's two resident point sets: 65536 bytes a share; 0 for a NULL handle */
size_t spz_commitment_resident_bytes(void* comm);
void spz_commitment_free(void* comm);

/* ---- assignments ---- */
/* VarsAssignment::new: nvars scalars uploaded once; proofs over the handle start from the device copy. NULL on failure. */
void* spz_vars_assignment_new(void* ctx, const uint64_t* vars, size_t nvars);
void spz_vars_assignment_free(void* assignment);
/* Assignment::new (lib.rs:62-88) as the reference takes it: 32 * n canonical little-endian bytes, in host memory (_from_bytes) or in the
 * memory of the context's device (_from_device_bytes: the caller has completed the writes), parsed on the device into an ordinary
 * resident assignment. NULL with spz_last_error() beginning "InvalidScalar" when an entry is >= q. report (may be NULL), on success and
 * on that failure alike: report[0] = entries >= q, report[1] = the lowest such index (UINT64_MAX when none). */
void* spz_vars_assignment_from_bytes(void* ctx, const uint8_t* bytes, size_t n, uint64_t report[2]);
void* spz_vars_assignment_from_device_bytes(void* ctx, const uint8_t* dev, size_t n, uint64_t report[2]);
size_t spz_vars_assignment_len(void* assignment); /* scalars held; 0 for a NULL handle */
/* Scalar::to_bytes of every entry: out receives 32 * spz_vars_assignment_len(a) bytes. 0 = ok, -1 = error. */
int spz_vars_assignment_to_bytes(void* assignment, uint8_t* out);
/* Are the resident limbs all < q (an assignment made from Montgomery limbs is taken on trust)? report as above, not NULL. 0 = checked,
 * -1 = error. */
int spz_vars_assignment_check_reduced(void* assignment, uint64_t report[2]);
/* The same parse for inputs and other short vectors, on the calling thread, no context: limbs_out receives 4 * n Montgomery limbs.
 * 0 = ok; -1 with spz_last_error() beginning "InvalidScalar" when an entry is >= q (limbs_out is then not written). report as above. */
int spz_scalars_from_bytes(const uint8_t* bytes, size_t n, uint64_t* limbs_out, uint64_t report[2]);
/* Scalar::to_bytes of n scalars: out receives 32 * n bytes. 0 = ok, -1 = error. */
int spz_scalars_to_bytes(const uint64_t* limbs, size_t n, uint8_t* out);

/* ---- proving ---- */
/* SNARK::prove / NIZK::prove. Each returns a proof handle (spz_proof_bytes, spz_proof_free), NULL on failure. Common arguments:
 *   gens           the PROVER's generators; a verifier-only handle is refused before any device call
 *   inputs         ninputs scalars
 *   tape_seed      4 limbs that seed the RandomTape, which then determines every blind: a test hook. NULL = seeded from OS entropy like
 *                  RandomTape::new (random.rs:13-15), the production setting
 *   times10        NULL, or 10 doubles that receive the seconds of the reference's timer spans
 * The assignment is host scalars read in place (spz_*_prove: vars, nvars), a resident handle (spz_*_prove_resident: assignment), or
 * either, the other NULL (spz_*_prove_t). The transcript is a fresh one made from transcript_label, or, in spz_*_prove_t, the CALLER'S
 * (lib.rs:339-347, 501-509: `transcript: &mut Transcript`): the 203 bytes of a merlin transcript (STROBE state, pos, pos_begin,
 * cur_flags) come in, the proof is produced on their continuation, and the state after the proof goes back so the caller's transcript
 * can carry on. spz_*_prove_t are the entries the Rust crate's SNARK::prove / NIZK::prove call under `--features gpu`. */
void* spz_snark_prove(void* ctx, void* inst, void* gens, void* enc, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                      const char* transcript_label, const uint64_t tape_seed[4], double* times10);
void* spz_snark_prove_resident(void* ctx, void* inst, void* gens, void* enc, void* assignment, const uint64_t* inputs, size_t ninputs,
                               const char* transcript_label, const uint64_t tape_seed[4], double* times10);
void* spz_snark_prove_t(void* ctx, void* inst, void* gens, void* enc, void* assignment, const uint64_t* vars, size_t nvars,
                        const uint64_t* inputs, size_t ninputs, uint8_t transcript_state[203], const uint64_t tape_seed[4], double* times10);
void* spz_nizk_prove(void* ctx, void* inst, void* gens, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                     const char* transcript_label, const uint64_t tape_seed[4], double* times10);
void* spz_nizk_prove_resident(void* ctx, void* inst, void* gens, void* assignment, const uint64_t* inputs, size_t ninputs,
                              const char* transcript_label, const uint64_t tape_seed[4], double* times10);
void* spz_nizk_prove_t(void* ctx, void* inst, void* gens, void* assignment, const uint64_t* vars, size_t nvars, const uint64_t* inputs,
                       size_t ninputs, uint8_t transcript_state[203], const uint64_t tape_seed[4], double* times10);
/* the bytes of a proof handle (bincode). Size, then fill. */
size_t spz_proof_bytes(void* proof, uint8_t* out, size_t cap);
void spz_proof_free(void* proof);
/* The layout probe of the coarse Rust binding (rust_shim/src/gpu_tail.rs.in), which reads and writes merlin::Transcript's private state
 * through the struct's memory: out_state = the 203 bytes after Transcript::new(b"spartan_amd binding probe") and
 * append_message(b"probe-message", 0..63); out_challenge = challenge_bytes(b"probe-challenge", 32) drawn from that state. The Rust side
 * runs the same script on its own transcript before its first use and panics on any difference. */
void spz_transcript_probe(uint8_t out_state[203], uint8_t out_challenge[32]);

/* ---- verifying ---- */
/* SNARK::verify (lib.rs:423-466) of untrusted proof bytes against a commitment handle (spz_commitment_load / _encode), and NIZK::verify
 * (lib.rs:549-587) against the instance: 1 accept, 0 reject, -1 malformed bytes, -2 error (spz_last_error(): "InvalidNumberOfInputs", bad
 * arguments, or a device failure). No argument may be NULL, except inputs when n_inputs is 0. The _t forms run on a caller-owned
 * transcript (see spz_*_prove_t): it is continued by the verification and left in the state it ends in. */
int spz_snark_verify(void* ctx, void* comm, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                     const char* transcript_label);
int spz_snark_verify_t(void* ctx, void* comm, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                       uint8_t transcript_state[203]);
int spz_nizk_verify(void* ctx, void* inst, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                    const char* transcript_label);
int spz_nizk_verify_t(void* ctx, void* inst, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                      uint8_t transcript_state[203]);
/* SNARK::verify_many / NIZK::verify_many: K untrusted proofs of one circuit (one instance) in lock step on the device, each under a
 * transcript of its own made from transcript_label; inputs[k] (n_inputs scalars) belongs to proofs[k]. Fills status_out[k] with 1 accept,
 * 0 reject, -1 malformed bytes and returns 0. Returns -2 with spz_last_error() for an error of the CALL: bad arguments, n_inputs that is
 * not the circuit's ("InvalidNumberOfInputs", before anything runs), a device failure; status_out is then all -2, so nothing is
 * reported as accepted. K = 0 is legal and does nothing: proofs, proof_lens, inputs and status_out may then be NULL. */
int spz_snark_verify_many(void* ctx, void* comm, void* gens, const uint8_t* const* proofs, const size_t* proof_lens,
                          const uint64_t* const* inputs, size_t n_inputs, size_t K, const char* transcript_label, int* status_out);
int spz_nizk_verify_many(void* ctx, void* inst, void* gens, const uint8_t* const* proofs, const size_t* proof_lens,
                         const uint64_t* const* inputs, size_t n_inputs, size_t K, const char* transcript_label, int* status_out);

/* ---- TEST HOOKS ----
 * Everything below exists for the tests and the measurement scripts: pieces of the driver's host side exposed one at a time so that they
 * can be compared with the oracle without a GPU. None of it is part of the product's API. */
/* No GPU, no context: deserialize untrusted bytes (SNARK, NIZK, ComputationCommitment), then serialize again. Returns the number of
 * bytes (written when cap suffices), -1 when malformed. */
long long spz_snark_reserialize(const uint8_t* proof, size_t len, uint8_t* out, size_t cap);
long long spz_nizk_parse_probe(const uint8_t* proof, size_t len, uint8_t* out, size_t cap);
long long spz_commitment_reserialize(const uint8_t* bytes, size_t len, uint8_t* out, size_t cap);
/* bincode(R1CSShape), which the digest compresses. Size, then fill. */
size_t spz_instance_shape_bincode(void* inst, uint8_t* out, size_t cap);
/* The deflater alone: the zlib stream of arbitrary bytes as miniz writes it at level 6, and at another tdefl probe count (miniz levels
 * 4..10 = 16/32/128/256/512/768/1500). Size, then fill. */
size_t spz_zlib_level6(const uint8_t* data, size_t n, int old_header, uint8_t* out, size_t cap);
size_t spz_zlib_probes(const uint8_t* data, size_t n, unsigned probes, int old_header, uint8_t* out, size_t cap);
/* The deflater's match search as one independent item per input position, and the parser over its tables (deflate.cc; the device runs the
 * same search: spartan_hip.h, sp_deflate_*). A table entry is dist | len << 16. spz_deflate_matches_host fills A and B (n entries each) and,
 * when L is not NULL, the hash-chain links L (n entries) on the calling thread: the CPU yardstick of the device search.
 * spz_zlib_from_matches runs tdefl's parser, block decisions and Huffman coding over such tables (L == NULL: the links are computed for
 * the lookups neither table answers) and returns spz_zlib_probes' bytes. Size, then fill; stats (may be NULL) = lookups, and how many of
 * them neither table answered. */
void spz_deflate_matches_host(const uint8_t* data, size_t n, unsigned probes, uint16_t* L, uint32_t* A, uint32_t* B);
size_t spz_zlib_from_matches(const uint8_t* data, size_t n, const uint16_t* L, const uint32_t* A, const uint32_t* B, unsigned probes,
                             int old_header, uint8_t* out, size_t cap, uint64_t stats[2]);
/* The whole device-assisted deflate of n bytes of host memory, as the digest runs it over bincode(shape): match search on the context's
 * device in segments of the option digest.segment, parser and coding on the calling thread behind it. Size, then fill (each call
 * compresses); 0 with spz_last_error() on failure. stats (may be NULL; 12 doubles): lookups, lookups neither table answered, segments, device
 * milliseconds of links / search A / search B / downloads, host milliseconds of parse and coding / waiting for the device / building the
 * stream / in total, and 1.0 when the device path ran. */
size_t spz_zlib_device(void* ctx, const uint8_t* data, size_t n, unsigned probes, int old_header, uint8_t* out, size_t cap, double stats[12]);
/* bincode(R1CSShape) with the matrices' part serialised on the device (sp_sparse_bincode): spz_instance_shape_bincode's bytes. Size, then
 * fill; 0 with spz_last_error() on failure. */
size_t spz_instance_shape_bincode_device(void* inst, uint8_t* out, size_t cap);
/* the figures of the instance's last digest computation, laid out as the stats of spz_zlib_device (the host path sets the total only) */
void spz_instance_digest_stats(void* inst, double stats[12]);
/* The parse restated as walks between the parser's free states, and the coder over its tokens (deflate.cc; the device runs the same parse:
 * spartan_hip.h, sp_deflate_tokens). A token is one 32-bit word per literal or match, in stream order: bit 31 set; bit 30 = tdefl's block
 * check runs after it; bit 29 = a match is held when that check runs; a literal has its byte in bits 0..7 and bits 15..23 zero, a match has
 * its length in bits 15..23 and dist - 1 in bits 0..14. spz_deflate_tokens_host writes up to n tokens and returns their number; geom (may be
 * NULL; 3) = tile, tiles a group and segment length of the device parse it models, which change no token, only the counters; counters (may be
 * NULL; 10) = walks, look-ups, look-ups neither match table answered, matches of >= 128 taken from a free state, a literal and a match of
 * >= 128 from one step, matches spanning a tile / a group boundary within a segment, segments entered with a held match, tokens, the longest
 * jump between two free states. spz_zlib_from_tokens codes such a list, `piece` tokens at a time (0: all at once), and returns
 * spz_zlib_probes' bytes. Size, then fill; blocks (may be NULL; 4) = blocks ended by the code-buffer rule, by the 115/128 rule, stored
 * blocks, static blocks. */
size_t spz_deflate_tokens_host(const uint8_t* data, size_t n, unsigned probes, const size_t* geom, uint32_t* tokens, uint64_t* counters);
size_t spz_zlib_from_tokens(const uint8_t* data, size_t n, const uint32_t* tokens, size_t ntok, unsigned probes, int old_header, size_t piece,
                            uint8_t* out, size_t cap, uint64_t* blocks);
/* spz_zlib_device with the form named: parse = 0 the parser on the host over downloaded match tables, 1 the parse on the device and the
 * token coder on the host, -1 what the option digest.device says (2 = the device parse); tile, group = positions a tile and tiles a group
 * of the device parse (0: 1024 and 64). stats (may be NULL) receives up to stats_cap of 17 doubles: the 12 of spz_zlib_device, then 1.0 when
 * the device parsed, tokens, look-ups the device searched on the spot, device milliseconds of the reachability kernels and of the token
 * kernel with its compaction. spz_instance_digest_stats_all: the same 17 of the instance's last digest computation. */
size_t spz_zlib_device_parse(void* ctx, const uint8_t* data, size_t n, unsigned probes, int old_header, int parse, size_t tile, size_t group,
                             uint8_t* out, size_t cap, double* stats, size_t stats_cap);
void spz_instance_digest_stats_all(void* inst, double* stats, size_t stats_cap);
/* The coder split as the device runs it with digest.device = 3 (deflate.cc; the device side: spartan_hip.h, sp_deflate_open_emit). A block
 * record is 6 words: index of the block's first token, its tokens, its input bytes, the rule that closed it (1 code buffer, 2 ratio,
 * 3 finish), and lookahead_pos - lz_dict_pos and dict_size of tdefl's stored-block test; beside it 320 16-bit counters, 288 of the
 * literal/length alphabet and 32 of the distances. spz_deflate_blocks_host finds the records of a token list of n input bytes segment by
 * segment (`segment` input positions; 0: one) as the device does and returns their number, at most cap, -1 with spz_last_error() for a
 * block of more than 58249 tokens; counters (may be NULL; 7) = blocks closed by the code-buffer rule, by the ratio rule, empty final
 * blocks, seams an open block was carried over, the most segments one block touched, blocks that end with a segment's last token, the
 * most tokens of a block. spz_zlib_from_blocks builds tables, headers and bit offsets from the histograms and ORs every token's bits in
 * at its offset: spz_zlib_probes' bytes. Size, then fill; stats (may be NULL; 3) = stored blocks, static blocks, stored blocks after a
 * block that ends within a byte. */
long long spz_deflate_blocks_host(const uint32_t* tokens, size_t ntok, size_t n, size_t segment, uint64_t* records, uint16_t* hist, size_t cap,
                                  uint64_t* counters);
size_t spz_zlib_from_blocks(const uint64_t* records, const uint16_t* hist, size_t nblocks, const uint32_t* tokens, const uint8_t* data, size_t n,
                            unsigned probes, int old_header, uint8_t* out, size_t cap, uint64_t* stats);
/* spz_zlib_device_parse with the third form: parse = 2 the coder's block boundaries, histograms, bit emission, stored-block copies and
 * Adler-32 on the device too (the calling thread builds the Huffman tables and bit offsets per block), -1 what digest.device says (3 = this
 * form); chunk = tokens a workgroup of the emission, 256..65536 (0: 4096). stats receives up to stats_cap of 26 doubles: the 17 of
 * spz_zlib_device_parse, then 1.0 when the device coded, the tokens it coded, blocks, stored blocks, static blocks, device milliseconds of the
 * block stage and of the bit emission, host milliseconds of the table building and of the download of the compressed bytes.
 * spz_instance_digest_stats_all reports the same 26. */
size_t spz_zlib_device_emit(void* ctx, const uint8_t* data, size_t n, unsigned probes, int old_header, int parse, size_t tile, size_t group, size_t chunk,
                            uint8_t* out, size_t cap, double* stats, size_t stats_cap);
/* Fiat-Shamir pieces. spz_keccak_run_variant: one permutation by the named form; 1 = ran, 0 = this CPU or build does not have it. */
int spz_keccak_run_variant(const char* name, uint64_t state[25]);
void spz_shake256(const uint8_t* in, size_t n, uint8_t* out, size_t outlen);
/* A script of nops operations on Transcript::new(tlabel): kinds[i] = 0 append_message(labels[i], datas[i], lens[i]), 1 challenge_bytes of
 * lens[i] bytes, 2 append_u64 of the 8 bytes at datas[i]. _script writes the challenges to out back to back and returns their total
 * length; _state writes the 203-byte state the script ends in (its challenges are drawn and dropped, at most 256 bytes each). */
size_t spz_merlin_script(const char* tlabel, size_t nops, const int* kinds, const char* const* labels, const uint8_t* const* datas,
                         const size_t* lens, uint8_t* out);
void spz_merlin_state(const char* tlabel, size_t nops, const int* kinds, const char* const* labels, const uint8_t* const* datas,
                      const size_t* lens, uint8_t out_state[203]);
/* continue a transcript from a state: one challenge of n bytes; the state is advanced in place */
void spz_merlin_challenge_from_state(uint8_t state[203], const char* label, uint8_t* out, size_t n);
/* n draws of RandomTape::new_with_seed("proof", seed).random_scalar(label): out receives 4 * n limbs */
void spz_tape_draws(const uint64_t seed[4], const char* label, size_t n, uint64_t* out);
/* TEST/BENCH ONLY: the reproducible 64-bit-seed -> scalar map behind the tape seeds of the tests and the benchmark */
void spz_seed_scalar(const char* domain, uint64_t seed, uint64_t out[4]);
/* Host arithmetic, Montgomery limbs in and out. spz_fq_invert_vartime: the challenge inversion of the inner-product rounds.
 * spz_unipoly_probe: UniPoly::from_evals / compress / evaluate (unipoly.rs) on n = 3 or 4 evaluations; 0 = ok, -1 = error.
 * spz_cubic_coeffs_probe, spz_cubic_tail_probe, spz_eq_factor_probe: the host side of the batched cubic sum-check. _tail: tab is
 * [ni][3][m], bound in place; evs receives 3 scalars a round; returns the number of rounds (log2 m). _eq_factor: 1 = ok, 0 = refused. */
void spz_fq_invert_vartime(const uint64_t in[4], uint64_t out[4]);
int spz_unipoly_probe(const uint64_t* evals, size_t n, const uint64_t r[4], uint64_t* coeffs, uint64_t* compressed, uint64_t eval_at_r[4]);
void spz_cubic_coeffs_probe(const uint64_t S[48], const uint64_t r[4], uint64_t ev[12]);
int spz_cubic_tail_probe(uint64_t* tab, size_t ni, size_t m, const uint64_t* coeffs, const uint64_t* challenges, uint64_t* evs);
int spz_eq_factor_probe(const uint64_t* rho, size_t nvars, size_t np, size_t ni, const uint64_t* coeffs, size_t nrounds, const uint64_t* claims,
                        const uint64_t* ev4, const uint64_t* challenges, uint64_t* evc_out, uint64_t* K_out);
/* microseconds per H2D + ncclAllGather + D2H + sync of `bytes` per rank over the context's RCCL transport; -2.0 = error */
double spz_rccl_allgather_probe(void* ctx, size_t bytes, int iters);

#ifdef __cplusplus
}
#endif
#endif
