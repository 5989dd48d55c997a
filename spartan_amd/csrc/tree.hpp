// spartan_amd: point-addition trees over LDS for a 256-thread block, every addition spread over the four lanes of a quad (device-inline:
// the MSM latency path and the reductions of commit.hip, the inner-product round of ipa.hip).
#pragma once
#include "curve.hpp"

// In-place LDS tree sum of sm[0..n) into sm[0] for a 256-thread block, with every point addition spread over FOUR lanes.
// A full extended addition is 9 dependent-ish field multiplications (~3.5 us for a lone lane); here lane `role` of a quad
// computes one of A = (Y1-X1)(Y2-X2), B = (Y1+X1)(Y2+X2), C = T1*(2d*T2), D = (2*Z1)*Z2, the quad exchanges them through
// LDS, and then one of X3 = E*F, Y3 = G*H, Z3 = F*G, T3 = E*H: three multiplications deep, same field elements (so the
// same canonical bytes). All roles run ONE instruction stream — operands are chosen by LDS address and by selects, never
// by branches — and the code is three multiplication bodies instead of nine (it is fetched cold by these few waves).
__device__ __forceinline__ Fe10 fe10_pick(const Fe10& a, const Fe10& b, bool take_b) { return fe10_select(a, b, take_b); }
// Hand-over between two tree levels that live in ONE wavefront (no block barrier): the LDS unit executes a wave's accesses in order, but
// the compiler sees no dependence between a lane's store of its sum and ANOTHER lane's load of it in the next level and may hoist that
// load; a workgroup-scope release/acquire fence pair plus a wave barrier pins the order in the instruction stream.
__device__ __forceinline__ void tree_wave_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Round 4 form: the four lanes of a quad are always lanes 4k..4k+3 of ONE wavefront, so A, B, C, D never need LDS or a barrier: they
// travel by DPP quad_perm moves (v_mov_b32 ... quad_perm:[..], 20 per addition).
//   stage 1   lane 0: A = (Y1-X1)(Y2-X2)   lane 1: B = (Y1+X1)(Y2+X2)   lane 2: C = T1 (2d T2)   lane 3: D = (2 Z1) Z2
//   swap with the neighbour (quad_perm [1,0,3,2]): lane 0: E = B - A   lane 1: H = B + A   lane 2: F = D - C   lane 3: G = D + C
//   fetch the second factor (quad_perm [1,3,0,2]): lane 0: T3 = E H    lane 1: Y3 = H G     lane 2: X3 = F E     lane 3: Z3 = G F
// The sum of a pair replaces its first point in LDS, written by the quad that read it (the LDS unit executes a wave's accesses in
// order, and no other quad touches those two points in this level), so a level needs ONE block barrier — before the next level reads
// points written by other wavefronts — and the levels of at most 16 additions, which live entirely in wavefront 0, need none.
// Same field elements as the round 1-3 form (A, B, C, D exchanged through LDS, three block barriers per level: measured against this one
// in round 4, DESIGN.md, and retired), hence the same canonical bytes. `xch` is unused (kept for the callers' LDS layout).
__device__ __forceinline__ Fe10 fe10_quad_perm_1032(const Fe10& a) {
  Fe10 r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = __builtin_amdgcn_mov_dpp(a.v[i], 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true);
  return r;
}
__device__ __forceinline__ Fe10 fe10_quad_perm_1302(const Fe10& a) {
  Fe10 r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = __builtin_amdgcn_mov_dpp(a.v[i], 0x8D /* quad_perm [1,3,0,2] */, 0xF, 0xF, true);
  return r;
}
__device__ __forceinline__ void pt10_tree_quad(Pt10* sm, Fe10* /*xch*/, size_t n) {
  const int t = threadIdx.x, role = t & 3;
  const Fe10 zero = Fe10{{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
  const Fe10 k2d = fe10_pick(fe10_one(), fe10_load(fp_D2()), role == 2);  // the factor 2d belongs to C only
  // field offsets inside Pt10, in units of Fe10: X 0, Y 1, Z 2, T 3
  const int fsel = role <= 1 ? 1 : (role == 2 ? 3 : 2);  // first field:  Y, Y, T, Z
  const int gsel = role <= 1 ? 0 : (role == 2 ? 3 : 2);  // second field: X, X, -, Z
  const int osel = role == 0 ? 3 : (role == 1 ? 1 : (role == 2 ? 0 : 2));  // coordinate this lane produces: T, Y, X, Z
  int top = 128;
  while (top > 1 && (size_t)top >= n) top >>= 1;  // no levels that would only add identities
  for (int s = top; s > 0; s >>= 1) {
    for (int base = 0; base < s; base += 64) {
      const int q = base + (t >> 2);
      const bool act = q < s && (size_t)(q + s) < n;
      if (act) {  // whole quads are active or not
        Fe10* P = reinterpret_cast<Fe10*>(sm + q);
        const Fe10* Q = reinterpret_cast<const Fe10*>(sm + q + s);
        Fe10 f1 = P[fsel], g1 = P[gsel], f2 = Q[fsel], g2 = Q[gsel];
        // role 0: f - g | role 1: f + g | role 2: f (T) | role 3: P: Z + Z, Q: Z
        g1 = fe10_pick(g1, fe10_neg(g1), role == 0);
        g1 = fe10_pick(g1, zero, role == 2);
        g2 = fe10_pick(g2, fe10_neg(g2), role == 0);
        g2 = fe10_pick(g2, zero, role >= 2);
        Fe10 u = fe10_add(f1, g1), v = fe10_add(f2, g2);
        Fe10 mine = fe10_mul(u, fe10_mul(v, k2d));               // A | B | C | D
        Fe10 other = fe10_quad_perm_1032(mine);                    // B | A | D | C
        Fe10 val = (role & 1) ? fe10_add(mine, other) : fe10_sub(other, mine);  // E | H | F | G
        Fe10 fac = fe10_quad_perm_1302(val);                       // H | G | E | F
        P[osel] = fe10_mul(val, fac);                              // T3 = E H | Y3 = H G | X3 = F E | Z3 = G F
      }
    }
    if (s > 16) __syncthreads();  // the next level pairs points written by other wavefronts (additions q and q + s/2 sit 4 s/2 >= 64 lanes apart)
    else tree_wave_handover();    // levels inside wavefront 0: the hardware orders a wave's LDS accesses, the COMPILER is told not to reorder them
  }
  __syncthreads();  // sm[0] is the sum for every thread of the block
}
// Round 4, second form: a tree level TWO multiplications deep instead of three. The unified addition above spends its third level of
// depth on the curve constant (C = T1 * (2d * T2)); the dedicated addition of Hisil-Wong-Carter-Dawson for a = -1 ("add-2008-hwcd-4")
// has no constant at all:
//   lane 0: A = (Y1-X1)(Y2+X2)   lane 1: B = (Y1+X1)(Y2-X2)   lane 2: C = (Z1+Z1) T2   lane 3: D = (T1+T1) Z2
//   swap with the neighbour:      lane 0: F = B - A   lane 1: G = B + A   lane 2: E = D + C   lane 3: H = D - C
//   fetch the second factor (quad_perm [1,3,0,2]):  lane 0: Z3 = F G   lane 1: Y3 = G H   lane 2: X3 = E F   lane 3: T3 = H E
// Same group element as the unified formula (a different projective representative), hence the same canonical bytes. The price is
// that the formula is not complete, and the tree pays it in two places:
//   * the neutral element (zero digits, lanes past the end: exactly (0, 1, 1, 0)) is never fed to it — `idf[i]` marks the points that
//     are the untouched neutral element; a sum with one is a copy, with two stays marked;
//   * P = Q (possible only when a caller-supplied generator list repeats a point under equal scalars; sums over disjoint sets of
//     independent generators cannot collide) gives F = H = 0 in identical limbs, i.e. the all-zero quadruple, which every later
//     addition — either formula — maps to the all-zero quadruple again: the ROOT then has Z = 0, which no valid point has, and the
//     host re-runs the launch with the unified tree (ipa.hip). P = -Q gives (0, Y, Z, 0) with Y = Z, a valid neutral element.
__device__ __forceinline__ void pt10_tree_quad_ded(Pt10* sm, unsigned char* idf, size_t n) {
  const int t = threadIdx.x, role = t & 3;
  const Fe10 zero = Fe10{{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
  // field offsets inside Pt10, in units of Fe10: X 0, Y 1, Z 2, T 3
  const int fP = role <= 1 ? 1 : role;                    // P: Y, Y, Z, T
  const int gP = role <= 1 ? 0 : role;                    //    X (minus for lane 0), X, Z, T
  const int fQ = role <= 1 ? 1 : (role == 2 ? 3 : 2);     // Q: Y, Y, T, Z
  const int osel = role == 0 ? 2 : (role == 1 ? 1 : (role == 2 ? 0 : 3));  // coordinate this lane produces: Z, Y, X, T
  int top = 128;
  while (top > 1 && (size_t)top >= n) top >>= 1;
  for (int s = top; s > 0; s >>= 1) {
    for (int base = 0; base < s; base += 64) {
      const int q = base + (t >> 2);
      const bool act = q < s && (size_t)(q + s) < n;
      if (act) {  // whole quads are active or not, and take the same branch below
        Fe10* P = reinterpret_cast<Fe10*>(sm + q);
        const Fe10* Q = reinterpret_cast<const Fe10*>(sm + q + s);
        const bool idP = idf[q] != 0, idQ = idf[q + s] != 0;
        if (!idQ) {
          if (idP) {
            P[role] = Q[role];
            if (role == 0) idf[q] = 0;
          } else {
            Fe10 f1 = P[fP], g1 = P[gP], f2 = Q[fQ], g2 = Q[0];
            g1 = fe10_pick(g1, fe10_neg(g1), role == 0);
            g2 = fe10_pick(fe10_pick(g2, fe10_neg(g2), role == 1), zero, role >= 2);
            Fe10 mine = fe10_mul(fe10_add(f1, g1), fe10_add(f2, g2));      // A | B | C | D
            Fe10 other = fe10_quad_perm_1032(mine);                         // B | A | D | C
            Fe10 minuend = fe10_pick(mine, other, role == 0), subtrahend = fe10_pick(other, mine, role == 0);
            Fe10 val = (role == 1 || role == 2) ? fe10_add(mine, other) : fe10_sub(minuend, subtrahend);  // F | G | E | H
            Fe10 fac = fe10_quad_perm_1302(val);                            // G | H | F | E
            P[osel] = fe10_mul(val, fac);                                   // Z3 = F G | Y3 = G H | X3 = E F | T3 = H E
          }
        }
      }
    }
    if (s > 16) __syncthreads();
    else tree_wave_handover();
  }
  __syncthreads();
}
// the untouched neutral element as the kernels build it: (0, 1, 1, 0) limb for limb (a computed neutral element has other limbs and is an
// ordinary operand)
__device__ __forceinline__ bool pt10_is_blank(const Pt10& p) {
  int32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) acc |= p.X.v[i] | p.T.v[i];
#pragma unroll
  for (int i = 1; i < 10; i++) acc |= p.Y.v[i] | p.Z.v[i];
  return acc == 0 && p.Y.v[0] == 1 && p.Z.v[0] == 1;
}
