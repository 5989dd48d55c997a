// TEST INFRASTRUCTURE (not part of the product): one element-wise wrapper per field / curve operation, shared by the host
// shim (hostcheck.cc, generic u128 forms) and the device microkernels (devcheck.hip, the device forms of field.hpp), so both
// run the very same plain C++ around the sp:: functions. Every wrapper reads two 32-byte operands and writes 32 bytes:
//   Fq    raw Montgomery limbs in and out
//   Fp    raw 4 x u64 limbs in (any value below 2^256), canonical bytes out (fp_to_bytes); *_raw: raw limbs out
//   Pt    compressed ristretto255 bytes in and out; a rejected encoding gives 32 bytes of 0xff (never a canonical encoding)
// ALT is the operation the other lanes of a wavefront run in the divergent mode of devcheck.hip.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../spartan_amd/csrc/msm.hpp"

namespace chk {
using namespace sp;

SP_HD Fq ld_fq(const uint8_t* p) { Fq x; memcpy(x.l, p, 32); return x; }
SP_HD Fp ld_fp(const uint8_t* p) { Fp x; memcpy(x.v, p, 32); return x; }
SP_HD void st_fq(const Fq& x, uint8_t* o) { memcpy(o, x.l, 32); }
SP_HD void st_fp_raw(const Fp& x, uint8_t* o) { memcpy(o, x.v, 32); }
SP_HD void st_bad(uint8_t* o) { for (int i = 0; i < 32; i++) o[i] = 0xff; }

#define CHK_OP(name) struct name { static SP_HD void run(const uint8_t* a, const uint8_t* b, uint8_t* o)
#define CHK_END }

CHK_OP(fq_add_op) { st_fq(fq_add(ld_fq(a), ld_fq(b)), o); } CHK_END;
CHK_OP(fq_sub_op) { st_fq(fq_sub(ld_fq(a), ld_fq(b)), o); } CHK_END;
CHK_OP(fq_neg_op) { (void)b; st_fq(fq_neg(ld_fq(a)), o); } CHK_END;
CHK_OP(fq_dbl_op) { (void)b; st_fq(fq_dbl(ld_fq(a)), o); } CHK_END;
CHK_OP(fq_mul_op) { st_fq(fq_mul(ld_fq(a), ld_fq(b)), o); } CHK_END;
CHK_OP(fq_sqr_op) { (void)b; st_fq(fq_sqr(ld_fq(a)), o); } CHK_END;
CHK_OP(fq_from_mont_op) { (void)b; st_fq(fq_from_mont(ld_fq(a)), o); } CHK_END;
CHK_OP(fq_to_mont_op) { (void)b; st_fq(fq_to_mont(ld_fq(a)), o); } CHK_END;
CHK_OP(fq_invert_op) { (void)b; st_fq(fq_invert(ld_fq(a)), o); } CHK_END;

CHK_OP(fp_add_op) { fp_to_bytes(fp_add(ld_fp(a), ld_fp(b)), o); } CHK_END;
CHK_OP(fp_sub_op) { fp_to_bytes(fp_sub(ld_fp(a), ld_fp(b)), o); } CHK_END;
CHK_OP(fp_neg_op) { (void)b; fp_to_bytes(fp_neg(ld_fp(a)), o); } CHK_END;
CHK_OP(fp_mul_op) { fp_to_bytes(fp_mul(ld_fp(a), ld_fp(b)), o); } CHK_END;
CHK_OP(fp_sqr_op) { (void)b; fp_to_bytes(fp_sqr(ld_fp(a)), o); } CHK_END;
CHK_OP(fp_invert_op) { (void)b; fp_to_bytes(fp_invert(ld_fp(a)), o); } CHK_END;
CHK_OP(fp_pow_p58_serial_op) { (void)b; fp_to_bytes(fp_pow_p58_serial(ld_fp(a)), o); } CHK_END;
CHK_OP(fp_add_raw_op) { st_fp_raw(fp_add(ld_fp(a), ld_fp(b)), o); } CHK_END;
CHK_OP(fp_sub_raw_op) { st_fp_raw(fp_sub(ld_fp(a), ld_fp(b)), o); } CHK_END;

CHK_OP(pt_recompress_op) { (void)b; Pt p; if (!pt_decompress(a, &p)) { st_bad(o); return; } pt_compress(p, o); } CHK_END;
CHK_OP(pt_add_op) { Pt p, q; if (!pt_decompress(a, &p) || !pt_decompress(b, &q)) { st_bad(o); return; } pt_compress(pt_add(p, q), o); } CHK_END;
CHK_OP(pt_dbl_op) { (void)b; Pt p; if (!pt_decompress(a, &p)) { st_bad(o); return; } pt_compress(pt_dbl(p), o); } CHK_END;
template <bool NEG>
SP_HD void pt_madd_run(const uint8_t* a, const uint8_t* b, uint8_t* o) {  // a +- b through the Niels entry pt_to_niels makes of b
  Pt p, q;
  if (!pt_decompress(a, &p) || !pt_decompress(b, &q)) { st_bad(o); return; }
  Niels n = pt_to_niels(q, fp_invert(q.Z));
  pt_compress(pt_madd(p, n, NEG), o);
}
CHK_OP(pt_madd0_op) { pt_madd_run<false>(a, b, o); } CHK_END;
CHK_OP(pt_madd1_op) { pt_madd_run<true>(a, b, o); } CHK_END;
// encode of a point with Z != 1: the coordinates of a scaled by z = the raw limbs of b (by d where those are 0 mod p)
CHK_OP(pt_compress_z_op) {
  Pt p;
  if (!pt_decompress(a, &p)) { st_bad(o); return; }
  Fp z = ld_fp(b);
  if (fp_is_zero(z)) z = fp_D();
  Pt s = {fp_mul(p.X, z), fp_mul(p.Y, z), fp_mul(p.Z, z), fp_mul(p.T, z)};
  pt_compress(s, o);
} CHK_END;

// X(name, operation, operation of the other lanes in divergent mode)
#define CHK_OPS(X)                                   \
  X(fq_add, fq_add_op, fq_sub_op)                    \
  X(fq_sub, fq_sub_op, fq_add_op)                    \
  X(fq_neg, fq_neg_op, fq_dbl_op)                    \
  X(fq_dbl, fq_dbl_op, fq_neg_op)                    \
  X(fq_mul, fq_mul_op, fq_add_op)                    \
  X(fq_sqr, fq_sqr_op, fq_dbl_op)                    \
  X(fq_from_mont, fq_from_mont_op, fq_neg_op)        \
  X(fq_to_mont, fq_to_mont_op, fq_dbl_op)            \
  X(fq_invert, fq_invert_op, fq_sqr_op)              \
  X(fp_add, fp_add_op, fp_sub_op)                    \
  X(fp_sub, fp_sub_op, fp_add_op)                    \
  X(fp_neg, fp_neg_op, fp_sqr_op)                    \
  X(fp_mul, fp_mul_op, fp_sub_op)                    \
  X(fp_sqr, fp_sqr_op, fp_neg_op)                    \
  X(fp_invert, fp_invert_op, fp_sqr_op)              \
  X(fp_pow_p58_serial, fp_pow_p58_serial_op, fp_mul_op) \
  X(fp_add_raw, fp_add_raw_op, fp_sub_raw_op)        \
  X(fp_sub_raw, fp_sub_raw_op, fp_add_raw_op)        \
  X(pt_recompress, pt_recompress_op, pt_dbl_op)      \
  X(pt_add, pt_add_op, pt_dbl_op)                    \
  X(pt_dbl, pt_dbl_op, pt_add_op)                    \
  X(pt_madd0, pt_madd0_op, pt_madd1_op)              \
  X(pt_madd1, pt_madd1_op, pt_madd0_op)              \
  X(pt_compress_z, pt_compress_z_op, pt_recompress_op)

}  // namespace chk
