// spartan_amd: row commitments: the latency-path kernels, reductions and encoders, the launch plan, and the sp_commit_rows* / sp_job_wait entry points.
// Host side: msm_plan decides every form (throughput form, the latency path's tree form, nblk, encode route), msm_launch dispatches on it;
// msm_enqueue_commit: the many-row enqueue, msm_tree1_enqueue: the one-block tree, msm_finish_few: the few-row ending; commit_args_ok, stage_blinds
// and stage_indexed serve the entry points.
#include "internal.hpp"
#include "tree.hpp"
#include <atomic>

// Latency path, fused form (rows <= SP_HOST_ENCODE_ROWS): grid (nblk, rows). Thread p of a row looks up the table entry
// of its (column, window) pair and the block sums its 256 entries in an LDS tree, so a Sigma-protocol commitment is ONE
// launch (nblk = 1, FINAL: the sum goes out as an extended point for the host to encode) and an inner-product round is two
// (Pt10 partials, then k_msm_reduce) instead of three. An affine table entry (y+x, y-x, 2dxy) becomes the extended point
// (2(yp-ym), 2(yp+ym), 4, (yp-ym)(yp+ym)) = 4*(x, y, 1, xy) with one multiplication.
template <bool FINAL>
__global__ void __launch_bounds__(256) k_msm_windows_tree(const Fq* __restrict__ Z, size_t z_row_stride, size_t cols,
                                                          const Niels* __restrict__ table, size_t g_off, const uint32_t* __restrict__ idx,
                                                          size_t idx_row_stride, const Fq* __restrict__ blinds, size_t h_idx,
                                                          void* __restrict__ out, MsmGeom geom) { SP_FG_PRIO();
  __shared__ Pt10 sm[256];
  __shared__ Fe10 xch[256];
  size_t ncol = cols + (blinds ? 1 : 0), P = ncol * geom.nwin, row = blockIdx.y;
  int t = threadIdx.x;
  size_t p = (size_t)blockIdx.x * 256 + t;
  Pt10 acc = pt10_identity();
  if (p < P) {
    size_t j = p % ncol;
    int w = (int)(p / ncol);
    Fq sc = j < cols ? ld_fq(Z + row * z_row_stride + j) : ld_fq(blinds + row);
    size_t pt = j < cols ? (idx ? (size_t)idx[row * idx_row_stride + j] : g_off + j) : h_idx;
    if (!fq_is_zero(sc)) {
      int d = msm_digit(fq_from_mont(sc), w, geom);
      if (d != 0) {
        Niels n = table[msm_tidx(geom, pt, w, d < 0 ? -d : d)];
        Fp dx = fp_sub(n.yp, n.ym), sy = fp_add(n.yp, n.ym);
        Fp X = fp_add(dx, dx), T = fp_mul(dx, sy);
        if (d < 0) { X = fp_neg(X); T = fp_neg(T); }
        acc = Pt10{fe10_load(X), fe10_load(fp_add(sy, sy)), Fe10{{4, 0, 0, 0, 0, 0, 0, 0, 0, 0}}, fe10_load(T)};
      }
    }
  }
  sm[t] = acc;
  __syncthreads();
  size_t live = P - (size_t)blockIdx.x * 256;  // partial indices of this block that exist
  pt10_tree_quad(sm, xch, live);
  if (t == 0) {
    Pt10 r = sm[0];
    if (FINAL) ((Pt*)out)[row] = Pt{fe10_to_fp(r.X), fe10_to_fp(r.Y), fe10_to_fp(r.Z), fe10_to_fp(r.T)};
    else ((Pt10*)out)[row * gridDim.x + blockIdx.x] = r;
  }
}
// The same lookups + tree for commitments of more than 256 (column, window) pairs per row (rows <= 8), in ONE launch: every
// workgroup leaves its partial sum in device memory and takes a ticket at its row's counter; the workgroup that draws the last
// ticket of a row adds the row's partial sums in a second tree and writes the row sum to the host-mapped page; the last
// workgroup of the launch raises the completion flag. (Before: lookups + tree, reduction and flag as three launches.)
__global__ void __launch_bounds__(256) k_msm_windows_tree_fused(const Fq* __restrict__ Z, size_t z_row_stride, size_t cols, const Niels* __restrict__ table,
                                                                size_t g_off, const uint32_t* __restrict__ idx, size_t idx_row_stride,
                                                                const Fq* __restrict__ blinds, size_t h_idx, Pt10* __restrict__ part, uint32_t* __restrict__ tickets,
                                                                Pt* __restrict__ sums_out, MsmGeom geom, DoneSig sig) { SP_FG_PRIO();
  __shared__ Pt10 sm[256];
  __shared__ Fe10 xch[256];
  __shared__ unsigned ticket;
  size_t ncol = cols + (blinds ? 1 : 0), P = ncol * geom.nwin, row = blockIdx.y;
  int t = threadIdx.x;
  size_t p = (size_t)blockIdx.x * 256 + t;
  Pt10 acc = pt10_identity();
  if (p < P) {
    size_t j = p % ncol;
    int w = (int)(p / ncol);
    Fq sc = j < cols ? ld_fq(Z + row * z_row_stride + j) : ld_fq(blinds + row);
    size_t pt = j < cols ? (idx ? (size_t)idx[row * idx_row_stride + j] : g_off + j) : h_idx;
    if (!fq_is_zero(sc)) {
      int d = msm_digit(fq_from_mont(sc), w, geom);
      if (d != 0) {
        Niels n = table[msm_tidx(geom, pt, w, d < 0 ? -d : d)];
        Fp dx = fp_sub(n.yp, n.ym), sy = fp_add(n.yp, n.ym);
        Fp X = fp_add(dx, dx), T = fp_mul(dx, sy);
        if (d < 0) { X = fp_neg(X); T = fp_neg(T); }
        acc = Pt10{fe10_load(X), fe10_load(fp_add(sy, sy)), Fe10{{4, 0, 0, 0, 0, 0, 0, 0, 0, 0}}, fe10_load(T)};
      }
    }
  }
  sm[t] = acc;
  __syncthreads();
  pt10_tree_quad(sm, xch, P - (size_t)blockIdx.x * 256);
  const unsigned nblk = gridDim.x;
  if (t == 0) {
    part[row * nblk + blockIdx.x] = sm[0];
    __threadfence();
    ticket = atomicAdd(tickets + row, 1u);
  }
  __syncthreads();
  if (ticket == nblk - 1) {
    __threadfence();
    Pt10 r = pt10_identity();
    bool any = false;
    for (size_t k2 = t; k2 < nblk; k2 += 256) {
      Pt10 q2 = part[row * nblk + k2];
      r = any ? pt10_add(r, q2) : q2;
      any = true;
    }
    __syncthreads();
    sm[t] = r;
    __syncthreads();
    pt10_tree_quad(sm, xch, nblk < 256 ? nblk : 256);
    if (t == 0) {
      Pt10 z = sm[0];
      sums_out[row] = Pt{fe10_to_fp(z.X), fe10_to_fp(z.Y), fe10_to_fp(z.Z), fe10_to_fp(z.T)};
      tickets[row] = 0;
    }
  }
  signal_done(sig);
}
// This kernel and its launcher stay in the unit of the other users of the unified tree (pt10_tree_quad): compiled in a unit without one
// the unified instantiation comes out with another schedule and register count (152 instead of 154 VGPRs), i.e. not the measured kernel.
// ---- one inner-product round in ONE launch (BulletReductionProof::prove, src/nizk/bullet.rs:72-100) ---------------------
// L = <a_L, G_R>, R = <a_R, G_L> over the ORIGINAL generators (spartan_hip.h: the folded generators are never built): row 0
// pairs scalar a'[i] s'[p] with generator p n_cur + h + i, row 1 scalar a'[h + i] s'[p] with generator p n_cur + i, for
// p < n0 / n_cur, i < h = n_cur / 2. The c_L Q + blind_L H part of each row (two terms) is added by the calling thread from
// its host-side window tables while this kernel runs (ipa.hip), so every column here is a plain generator column.
// Blocks [0, 2 nblk): 256 (column, window) lookups of one row each, summed in the LDS tree; the block that arrives last at
// its row's counter adds the row's nblk partial sums and writes the row sum to the host-mapped page — what used to be three
// launches (scalar rows, lookups + tree, reduction) and a flag kernel. With `fold` set the vectors are those of the previous
// round and the fold of bullet.rs:105-109 by (u, u^-1) is applied on the way (a' = a_L u + u^-1 a_R, s'[2p] = s[p] u^-1,
// s'[2p+1] = s[p] u: 3 multiplications per lookup, redundantly per window, instead of a launch of their own).
// Blocks [2 nblk, 2 nblk + nd) work off the critical path: they materialise a', b', s' for the next round and form the eight
// quarter dot products from which the NEXT round's c_L, c_R follow once its challenge is known:
//   c_L'' = <a'_LL,b'_LR> + u^2 <a'_LL,b'_RR> + u^-2 <a'_RL,b'_LR> + <a'_RL,b'_RR>
//   c_R'' = <a'_LR,b'_LL> + u^2 <a'_LR,b'_RL> + u^-2 <a'_RR,b'_LL> + <a'_RR,b'_RL>        (quarters of a', b' in index order LL, LR, RL, RR)
// so no round waits for a dot product over the whole vectors (bullet.rs:80-81).
__device__ __forceinline__ Fq ipa_fold_a(const Fq* __restrict__ a, size_t x, size_t n_cur, int fold, const Fq& u, const Fq& u_inv) {
  Fq v = ld_fq(a + x);
  return fold ? fq_add(fq_mul(v, u), fq_mul(u_inv, ld_fq(a + n_cur + x))) : v;  // a' = a_L u + u^-1 a_R
}
__device__ __forceinline__ Fq ipa_fold_b(const Fq* __restrict__ b, size_t x, size_t n_cur, int fold, const Fq& u, const Fq& u_inv) {
  Fq v = ld_fq(b + x);
  return fold ? fq_add(fq_mul(v, u_inv), fq_mul(u, ld_fq(b + n_cur + x))) : v;  // b' = b_L u^-1 + u b_R
}
template <bool DED>  // DED: the two-multiplication tree level (pt10_tree_quad_ded); false: the unified formula (the fallback of an exceptional sum)
__global__ void __launch_bounds__(256) k_ipa_round(IpaRoundArgs A, const Niels* __restrict__ table, MsmGeom geom, DoneSig sig) { SP_FG_PRIO();
  __shared__ Pt10 sm[256];
  __shared__ Fe10 xch[256];
  __shared__ unsigned ticket;
  unsigned char* const idf = reinterpret_cast<unsigned char*>(xch);  // DED: one mark per point (the unified tree's exchange buffer is unused then)
  const int t = threadIdx.x;
  const size_t h = A.n_cur / 2;
  if (blockIdx.x >= 2 * A.nblk) {
    // ---- the next round's vectors and quarter dot products
    Fq* const red = reinterpret_cast<Fq*>(sm);  // [8][64]
    const size_t qlen = A.n_cur >= 4 ? A.n_cur / 4 : 1;
    const unsigned db = blockIdx.x - 2 * A.nblk;
    const size_t z = (size_t)db * 64 + (t >> 2);
    const int k = t & 3;
    const size_t x = z + (size_t)k * qlen;
    const bool live = z < qlen && x < A.n_cur;
    Fq av = fq_zero(), bv = fq_zero();
    if (live) {
      av = ipa_fold_a(A.a, x, A.n_cur, A.fold, A.u, A.u_inv);
      bv = ipa_fold_b(A.b, x, A.n_cur, A.fold, A.u, A.u_inv);
      if (A.fold) { st_fq(A.a_new + x, av); st_fq(A.b_new + x, bv); }
      // the last round (two entries left): a', b' also go to the host page, behind the dot-product slots — with them, the round's two raw row
      // sums and the last challenge the calling thread finishes the argument itself (ipa.hip, sp_ipa_finish_commit)
      if (A.n_cur == 2) { st_fq(A.dots_out + 8 + x, av); st_fq(A.dots_out + 10 + x, bv); }
    }
    if (A.fold)
      for (size_t p = (size_t)db * 256 + t; p < A.n0 / A.n_cur; p += (size_t)A.nd * 256)
        st_fq(A.s_new + p, fq_mul(ld_fq(A.s + p / 2), (p & 1) ? A.u : A.u_inv));  // s'[2p] = s[p] u^-1, s'[2p+1] = s[p] u
    // lane k of an index multiplies its a' with two of the b' of the index: exchange the b' through LDS
    Fq* const bx = reinterpret_cast<Fq*>(xch);  // [64][4]
    bx[(t >> 2) * 4 + k] = bv;
    __syncthreads();
    Fq e0 = fq_zero(), e1 = fq_zero();
    if (live && A.n_cur >= 4) {
      e0 = fq_mul(av, bx[(t >> 2) * 4 + ((k & 1) ? 0 : 1)]);
      e1 = fq_mul(av, bx[(t >> 2) * 4 + ((k & 1) ? 2 : 3)]);
    }
    // dot d = 2 * slot(k) + {0, 1} with slot: k = 0 (a_LL) -> d0, d1 | k = 2 (a_RL) -> d2, d3 | k = 1 (a_LR) -> d4, d5 | k = 3 (a_RR) -> d6, d7
    const int slot = k == 0 ? 0 : (k == 2 ? 1 : (k == 1 ? 2 : 3));
    __syncthreads();
    red[(2 * slot) * 64 + (t >> 2)] = e0;
    red[(2 * slot + 1) * 64 + (t >> 2)] = e1;
    __syncthreads();
    for (int st = 32; st > 0; st >>= 1) {
      for (int v = t; v < 8 * st; v += 256) {
        const int d = v / st, i = v % st;
        red[d * 64 + i] = fq_add(red[d * 64 + i], red[d * 64 + i + st]);
      }
      __syncthreads();
    }
    if (t < 8) st_fq(A.dots_out + (size_t)db * 8 + t, red[t * 64]);
    signal_done(sig);
    return;
  }
  // ---- lookups of one row + tree
  const unsigned row = blockIdx.x / A.nblk, blk = blockIdx.x % A.nblk;
  DoneSig kt0 = sig; if (blockIdx.x != 0) kt0.kt = nullptr;   // stamps 0..5: the first workgroup
  SP_KT(kt0, 0);
  const size_t cols = A.n0 / 2, P = cols * (size_t)geom.nwin;
  const size_t p = (size_t)blk * 256 + t;
  Pt10 acc = pt10_identity();
  if (p < P) {
    const size_t q = p % cols;
    const int w = (int)(p / cols);
    const size_t pb = q / h, i = q % h;
    const size_t gen = A.g_off + pb * A.n_cur + (row == 0 ? h + i : i);
    // a'[x] s'[p] with the pending fold applied: (a_L u + a_R u^-1) * s[p/2] u^(+-1) = s[p/2] (a_L u^2 + a_R) for odd p, s[p/2] (a_L + a_R u^-2) for
    // even p — two multiplications per lookup instead of four (the same field element)
    const size_t x = row == 0 ? i : h + i;
    Fq sc;
    if (A.fold) {
      const Fq aL = ld_fq(A.a + x), aR = ld_fq(A.a + A.n_cur + x);
      const Fq t = (pb & 1) ? fq_add(fq_mul(aL, A.u2), aR) : fq_add(aL, fq_mul(aR, A.u2_inv));
      sc = fq_mul(ld_fq(A.s + pb / 2), t);
    } else {
      sc = fq_mul(ld_fq(A.a + x), ld_fq(A.s + pb));
    }
    SP_KT(kt0, 1);
    if (!fq_is_zero(sc)) {
      int d = msm_digit(fq_from_mont(sc), w, geom);
      if (d != 0) {
        Niels n = table[msm_tidx(geom, gen, w, d < 0 ? -d : d)];
        SP_KT(kt0, 2);
        Fp dx = fp_sub(n.yp, n.ym), sy = fp_add(n.yp, n.ym);
        Fp X = fp_add(dx, dx), T = fp_mul(dx, sy);
        if (d < 0) { X = fp_neg(X); T = fp_neg(T); }
        acc = Pt10{fe10_load(X), fe10_load(fp_add(sy, sy)), Fe10{{4, 0, 0, 0, 0, 0, 0, 0, 0, 0}}, fe10_load(T)};
      }
    }
  }
  sm[t] = acc;
  if (DED) idf[t] = pt10_is_blank(acc) ? 1 : 0;
  SP_KT(kt0, 3);
  __syncthreads();
  if (DED) pt10_tree_quad_ded(sm, idf, P - (size_t)blk * 256);
  else pt10_tree_quad(sm, xch, P - (size_t)blk * 256);
  SP_KT(kt0, 4);
  if (t == 0) {
    A.part[(size_t)row * A.nblk + blk] = sm[0];
    __threadfence();  // the partial sum is visible device-wide before this block counts itself in
    ticket = atomicAdd(A.counters + row, 1u);
  }
  __syncthreads();
  SP_KT(kt0, 5);
  if (ticket == A.nblk - 1) {  // last block of the row: add the row's partial sums
    DoneSig kt1 = sig; if (row != 0) kt1.kt = nullptr;   // stamps 8..11: the reducing workgroup of row 0
    SP_KT(kt1, 8);
    __threadfence();
    Pt10 r = pt10_identity();
    bool any = false;
    for (size_t k2 = t; k2 < A.nblk; k2 += 256) {
      Pt10 q2 = A.part[(size_t)row * A.nblk + k2];
      r = any ? pt10_add(r, q2) : q2;
      any = true;
    }
    __syncthreads();
    sm[t] = r;
    if (DED) idf[t] = pt10_is_blank(r) ? 1 : 0;
    SP_KT(kt1, 9);
    __syncthreads();
    if (DED) pt10_tree_quad_ded(sm, idf, A.nblk < 256 ? A.nblk : 256);
    else pt10_tree_quad(sm, xch, A.nblk < 256 ? A.nblk : 256);
    SP_KT(kt1, 10);
    if (t == 0) {
      Pt10 z = sm[0];
      A.sums_out[row] = Pt{fe10_to_fp(z.X), fe10_to_fp(z.Y), fe10_to_fp(z.Z), fe10_to_fp(z.T)};
      A.counters[row] = 0;
    }
    SP_KT(kt1, 11);
  }
  signal_done(sig);
}
// unified: the tree with the complete addition formula (the re-run of a round whose row sum came back with Z = 0; ipa.unified_tree = 1 selects it
// for every round: the A/B switch)
int32_t ipa_round_launch(sp_ctx* c, const sp_gens* g, IpaRoundArgs* A, DoneSig* sig_out, int unified) {
  const size_t P = (A->n0 / 2) * (size_t)g->geom.nwin;
  A->nblk = (unsigned)((P + 255) / 256);
  const size_t qlen = A->n_cur >= 4 ? A->n_cur / 4 : 1;
  A->nd = (unsigned)((qlen + 63) / 64);
  if (1024 + ((size_t)A->nd * 8 + 4) * 32 > HOST_SUM_BYTES) return SP_EINVAL;  // the dot-product partials share the host page with the two row sums (n_cur <= 16384)
  SPCHK(ensure(&c->scratch, &c->scratch_cap, sizeof(Pt10) * 2 * (size_t)A->nblk + 256));
  A->part = (Pt10*)c->scratch;
  A->sums_out = (Pt*)hres(c);
  A->dots_out = (Fq*)(hres(c) + 1024);
  DoneSig sig = sig_make(c, 2 * (size_t)A->nblk + A->nd);
  {
    ProfScope ps(c, PF_IPA, 32.0 * 3 * (double)A->n0 + 160.0 * 2 * (double)A->nblk, nullptr, (double)(2 * P));
    // The dedicated (two-multiplication) tree is incomplete, and its exceptional pairs are detected at the root only for P = Q and
    // P = Q + (0, -1) (an all-zero quadruple propagates to Z = 0); for Q = P +- (i, 0) the formula gives Y3 = Z3 = 0 with X3 != 0, which a
    // later addition can turn back into Z != 0 — undetected. Such pairs need a known relation between partial
    // sums over disjoint generators: impossible for points the library derived itself by hash-to-curve (MultiCommitGens::new), possible in
    // principle for a caller-supplied list (sp_gens_upload). Caller-supplied sets therefore always get the complete (unified) tree.
    const bool always_unified = c->opt.v[OPT_IPA_UNIFIED_TREE] != 0 || (!g->derived && !c->opt.v[OPT_IPA_DEDICATED_UPLOADED]);
    if (unified || always_unified) hipLaunchKernelGGL(k_ipa_round<false>, dim3(2 * A->nblk + A->nd), dim3(256), 0, c->stream, *A, (const Niels*)g->table, g->geom, sig);
    else hipLaunchKernelGGL(k_ipa_round<true>, dim3(2 * A->nblk + A->nd), dim3(256), 0, c->stream, *A, (const Niels*)g->table, g->geom, sig);
  }
  *sig_out = sig;
  return hipGetLastError() == hipSuccess ? SP_OK : SP_EHIP;
}

// reduction pass: grid (rows, nchunks); block sums `chunk` consecutive partials of its row into one point.
// Reductions run on the radix-2^25.5 serial-chain arithmetic (fe10.hpp): few waves, latency-bound.
__global__ void __launch_bounds__(256) k_pt_reduce_pass(const Pt* __restrict__ in, size_t P, size_t chunk, Pt10* __restrict__ out,
                                                        const unsigned* __restrict__ counts /* queue form: slots in use per 64-row group, or null */) { SP_FG_PRIO();
  __shared__ Pt10 sm[256];
  __shared__ Fe10 xch[256];
  size_t row = blockIdx.x, ck = blockIdx.y, nchunks = gridDim.y;
  int t = threadIdx.x;
  size_t lo = ck * chunk, hi = lo + chunk;
  if (hi > P) hi = P;
  if (counts && hi > counts[row / 64]) hi = counts[row / 64];
  Pt10 acc = pt10_identity();
  bool any = false;
  for (size_t s = lo + t; s < hi; s += 256) {
    Pt10 p = pt10_load(in[row * P + s]);
    acc = any ? pt10_add(acc, p) : p;
    any = true;
  }
  sm[t] = acc;
  __syncthreads();
  pt10_tree_quad(sm, xch, 256);
  if (t == 0) out[row * nchunks + ck] = sm[0];
}
// one block per row: sum the row's partials, RFC 9496 encode. IN10: partials already in Pt10 form (second pass).
// ENCODE = false: the sum is written as an extended point (4 x 32 B, canonical coordinates) and the caller encodes it on
// the host. The encode is ONE serial chain of ~265 field multiplications (an inverse square root): ~100 us for a lone
// wavefront at one instruction per ~5 cycles, ~3 us for a CPU core with a 64-bit multiplier. Commitments of a few rows
// (every Sigma-protocol and inner-product round: 151 sequential ones per 2^20 proof) take the host route, batched row
// commitments (hundreds of rows in parallel) the device route.
template <bool IN10, bool ENCODE>
__global__ void __launch_bounds__(256) k_msm_reduce(const void* __restrict__ partial_, size_t nstrips, uint8_t* __restrict__ out,
                                                    const unsigned* __restrict__ counts /* queue form: slots in use per 64-row group, or null */) { SP_FG_PRIO();
  __shared__ Pt10 sm[256];
  __shared__ Fe10 xch[256];
  size_t row = blockIdx.x;
  int t = threadIdx.x;
  Pt10 acc = pt10_identity();
  bool any = false;
  size_t nlive = nstrips;  // the row's partial sums lie nstrips apart; the first nlive of them hold a sum
  if (counts && !IN10 && counts[row / 64] < nstrips) nlive = counts[row / 64];
  for (size_t s = t; s < nlive; s += 256) {
    Pt10 p = IN10 ? ((const Pt10*)partial_)[row * nstrips + s] : pt10_load(((const Pt*)partial_)[row * nstrips + s]);
    acc = any ? pt10_add(acc, p) : p;
    any = true;
  }
  sm[t] = acc;
  __syncthreads();
  pt10_tree_quad(sm, xch, nlive < 256 ? nlive : 256);
  if (t == 0) {
    Pt10 r = sm[0];
    if (ENCODE) {
      uint8_t c[32];
      fe10_pin(r.X); fe10_pin(r.Y); fe10_pin(r.Z); fe10_pin(r.T);
      pt10_compress(r, c);
      for (int k = 0; k < 32; k++) out[32 * row + k] = c[k];
    } else {
      ((Pt*)out)[row] = Pt{fe10_to_fp(r.X), fe10_to_fp(r.Y), fe10_to_fp(r.Z), fe10_to_fp(r.T)};
    }
  }
}


// RFC 9496 encode of many row sums at once: one LANE per row. (With the encode inside k_msm_reduce one lane per BLOCK runs
// the ~100 us inverse-square-root chain while 255 wait: a 1024-row commit spent 0.6 ms there; this way the 1024 chains
// run side by side in 16 wavefronts.)
__device__ __forceinline__ void pt_encode_rows(const Pt* __restrict__ in, size_t rows, uint8_t* __restrict__ out) {
  size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= rows) return;
  uint8_t c[32];
  pt10_compress(pt10_load(in[row]), c);
  for (int k = 0; k < 32; k++) out[32 * row + k] = c[k];
}
__global__ void __launch_bounds__(64) k_pt_encode(const Pt* __restrict__ in, size_t rows, uint8_t* __restrict__ out) { SP_FG_PRIO();
  pt_encode_rows(in, rows, out);
}
// The same in at most 168 VGPRs (the compiler takes all 256 for its schedule of the chain above; here it spills ~100 dwords): the encode of
// the ROW half of `derefs` runs while the column half's queue-form MSM holds two wavefronts per SIMD on every CU — 272 of a lane's 512
// registers — and a 256-register wavefront could not be placed until that launch had ended (first round-6 traces: k_pt_encode 0.13 -> 3 ms
// on average at 2^22, the row half's shares absorbed after the MSM instead of under it).
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) k_pt_encode_lean(const Pt* __restrict__ in, size_t rows, uint8_t* __restrict__ out) { SP_FG_PRIO();
  pt_encode_rows(in, rows, out);
}

// (The kernels above keep their repeated text on purpose: with the lookup, the tree kernels' front, the strided sum or the last-ticket tail as
// __forceinline__ helpers, every kernel that used one came out with another register allocation or instruction count: not the measured kernels.)
// MSM launch plan: kernel shapes and scratch sizes for a (rows x cols) fixed-base commit
// (the latency path's tree forms: one workgroup per row, its sum final | more, the last of a row adds them | more, k_msm_reduce adds them)
enum { MSM_TREE_NONE = 0, MSM_TREE1, MSM_TREE_FUSED, MSM_TREE_UNFUSED };
struct MsmPlan {
  bool windowed, two_pass;
  bool lds = false;  // the LDS-staged small-window form (msm_lds.hip), P = runs per row-block
  bool queue = false; // the queue form (msm_queue.hip, k_msm_q): P = runs per row
  MsmQRuns qruns{0, 0, 0};
  int qrole = MSMQ_ALONE;
  int flat;  // 0: strip form; 2: balanced form (k_msm_flat), P = runs per row
  size_t strip, nstrips, P, chunk, nchunks, part_bytes, part2_bytes;
  // msm_launch's latency path (few; a job reads none of this): its tree form (none: the sums above + k_msm_reduce), the tree's workgroups per row,
  // and whether k_pt_encode runs the encode chain (encode.device) instead of the host core
  bool few = false, encode_dev = false;
  int tree = MSM_TREE_NONE;
  size_t nblk = 0;
};
// (c: the LAUNCHING context — options, CU count and background share are its own; a virtual shard launches its parent's generator set)
static MsmPlan msm_plan(const sp_ctx* c, const sp_gens* g, size_t rows, size_t cols, bool has_blinds, size_t bg_subblocks = 0 /* background launch: 256-thread tiles it runs at once */,
                        size_t launch_rows = 0 /* rows per launch when the commit is issued in row chunks (sp_commit_rows_upload_start) */,
                        bool shares_chip = false /* a background commit of this context is in flight */) {
  MsmPlan m;
  m.flat = 0;
  const size_t NWIN = (size_t)g->geom.nwin;
  size_t total = rows * cols, ncol = cols + (has_blinds ? 1 : 0);
  m.windowed = rows * ncol * NWIN <= ((size_t)1 << 19);  // latency-bound shapes: one addition per thread
  m.strip = 1; m.nstrips = 0;
  if (m.windowed) {
    m.P = ncol * NWIN;
  } else {
    const SpOptions& opt = c->opt;
    const size_t target_threads = 524288;  // (256 k and 1 M threads measured in round 3: both slower)
    m.strip = total / target_threads;  // enough threads for >= 4 waves per SIMD on 256 CUs
    if (m.strip < 1) m.strip = 1;
    if (m.strip > cols) m.strip = cols;
    m.nstrips = (cols + m.strip - 1) / m.strip;
    m.P = m.nstrips;
    if (launch_rows == 0) launch_rows = rows;
    // balanced form: a launch of at most four row-blocks that has the chip to itself (the witness commitment and its upload chunks,
    // stand-alone commits of few rows). Everything else that is not queue-sized keeps the strip form: the background launch (its
    // balanced form finished a 768 x 4096 commit in 4.7 instead of 5.8 ms on 5/8 of the chip and the latency-bound kernels next to it then
    // ran 2x slower instead of 1.3x: profiles/r4_ab_msm_forms.txt), a foreground commit that shares the chip with a background one (the
    // balanced form is exactly as many workgroups as an EMPTY chip holds, each as long as the launch), and a commit of many row-blocks
    // whose rows carry unlike scalars (equal additions per workgroup are equal time only when the scalars are alike)
    if (rows % 256 == 0 && launch_rows % 256 == 0 && launch_rows / 256 <= 4 && !bg_subblocks && !shares_chip) {
      const size_t rb = launch_rows / 256, units = ncol * NWIN;
      size_t nb = msm_flat_slots() / rb;        // runs per row: the launch is one full set of resident workgroups
      if (nb > units / 4) nb = units / 4;       // at least four additions per thread
      if (nb >= 1) { m.flat = 2; m.P = nb; }
    }
    if (opt.v[OPT_MSM_FORM] == 1 && !g->table_lds) {  // asked for, not possible: say so once instead of silently measuring another form
      static std::atomic<bool> warned{false};
      if (!warned.exchange(true)) fprintf(stderr, "spartan_hip: msm.form = 1 but the generator set was built without LDS-form tables (set msm.lds_bits before creating it): its row commitments take the default forms\n");
    }
    // LDS-staged small-window form: a workgroup is up to 1024 rows, so it needs rows to fill a CU with (>= 768 for 3 waves per SIMD)
    if (g->table_lds && (opt.v[OPT_MSM_FORM] == 1 || (opt.v[OPT_MSM_FORM] == 0 && g->prefer_lds)) && launch_rows >= 512) {
      const size_t cus = (size_t)c->n_cus;
      // one workgroup per CU (96 KB of LDS each); next to a background commit the launch is cut three times finer, so that the CUs
      // the background job leaves free are handed runs as they come
      size_t slots = bg_subblocks ? bg_subblocks / 4 : (shares_chip ? 3 * cus : cus);
      m.lds = true; m.flat = 0;
      m.P = msm_lds_runs(g, launch_rows, cols, has_blinds, slots);
    } else if ((opt.v[OPT_MSM_FORM] == 0 || opt.v[OPT_MSM_FORM] == 2) && launch_rows >= 256 && launch_rows == rows && (rows + 63) / 64 <= MSMQ_MAX_GROUPS) {
      // THE DEFAULT for commits of >= 256 rows since round 6: the queue form (msm_queue.hip). Measured against the strip / balanced forms it
      // replaces there (profiles/r6_ab_queue_form.txt): 8-18 % faster per launch, SNARK::prove 2^20 -0.6 ms; msm.form = 3 keeps the old forms.
      // (a commit issued in row chunks behind its upload has the chip to itself and rows that are alike: the balanced form's case)
      m.queue = true; m.flat = 0;
      // the background launch and a foreground launch that meets one in flight share the chip with each other and with the latency kernels
      m.qrole = bg_subblocks || shares_chip ? MSMQ_CORESIDENT : MSMQ_ALONE;
      m.qruns = msm_q_cut(c, g, launch_rows, cols, has_blinds, m.qrole);
      m.P = m.qruns.S;
    }
  }
  m.chunk = 1024; m.nchunks = (m.P + m.chunk - 1) / m.chunk;
  m.two_pass = m.P > 2048;
  m.part_bytes = (rows * m.P * sizeof(Pt) + 255) & ~(size_t)255;
  m.part2_bytes = m.two_pass ? ((rows * m.nchunks * sizeof(Pt10) + 255) & ~(size_t)255) : 0;
  if (rows <= SP_HOST_ENCODE_ROWS) {  // latency path: the device sums, the host core runs the encode chain
    // (encode.device: the sums stay in device memory and k_pt_encode runs the chain there — same bytes, ~100 us later)
    m.few = true;
    m.encode_dev = c->device_encode;
    if (m.windowed) {
      size_t nblk = (m.P + 255) / 256;  // nblk * rows * 160 B of partial sums <= part_bytes
      m.nblk = nblk;
      m.tree = nblk == 1 ? MSM_TREE1 : MSM_TREE_UNFUSED;
      if (nblk > 1 && !c->device_encode && c->done_counter) {
        m.tree = MSM_TREE_FUSED;  // one launch, its flag waited for
      }
    }
  }
  return m;
}
// scratch of one commit: [partials: part_bytes][second-pass partials: part2_bytes][32 B x rows encodings, padded to 256][row sums as points]
struct MsmScratch { size_t out_off, sums_off, bytes; };
static MsmScratch msm_scratch(const MsmPlan& m, size_t rows) {
  const size_t out_off = m.part_bytes + m.part2_bytes, out_al = (32 * rows + 255) & ~(size_t)255;
  return MsmScratch{out_off, out_off + out_al, out_off + out_al + sizeof(Pt) * rows};
}
// enqueue the lookups of one commit on `st`: partial sums into scratch (part_bytes). Returns the queue form's partial-sum slots in use per
// 64-row group (device) for the reduction that follows, null for the other forms
static const unsigned* msm_enqueue_sums(sp_ctx* c, hipStream_t st, const MsmPlan& m, const sp_gens* g, const Fq* dZ, size_t z_stride, size_t rows,
                                        size_t cols, size_t g_off, const uint32_t* didx, const Fq* dblinds, size_t h_idx, uint8_t* scratch) {
  size_t total = rows * cols;
  Pt* partial = (Pt*)scratch;
  const unsigned* qcounts = nullptr;
  if (m.windowed) {
    ProfScope ps(c, PF_MSM_WINDOWS, 32.0 * (double)total + 128.0 * (double)(rows * m.P), st);  // HIP events on the stream the kernels run on
    msm_rows_enqueue(c, st, g, dZ, z_stride, rows, cols, g_off, didx, dblinds, h_idx, partial, MSM_ROWS_WINDOWS, 0, m.P);
  } else {
    // K1: 32 B read per committed scalar + 32 B written per row
    // ops: mixed additions if no scalar is zero; shape key: rows | cols | background launch
    uint64_t shape = ((uint64_t)rows << 32) | (uint64_t)cols | (st != c->stream ? (1ULL << 63) : 0);
    ProfScope ps(c, PF_MSM_ROWS, 32.0 * (double)total + 32.0 * (double)rows, st, (double)total * g->geom.nwin, shape);
    if (m.queue) {
      msm_q_enqueue(c, st, g, dZ, z_stride, rows, cols, g_off, didx, dblinds, h_idx, partial, m.qruns, m.qrole, &qcounts, &ps.issued);
    } else if (m.lds) {
      msm_lds_enqueue(c, st, g, dZ, z_stride, rows, cols, g_off, didx, dblinds, h_idx, partial, m.P, st != c->stream && c->bg_blocks > 0 ? (unsigned)c->bg_blocks : 0u);
    } else {
      msm_rows_enqueue(c, st, g, dZ, z_stride, rows, cols, g_off, didx, dblinds, h_idx, partial, m.flat ? MSM_ROWS_FLAT : MSM_ROWS_STRIP, m.strip, m.P);
    }
  }
  return qcounts;
}
// enqueue the reduction of the partial sums in scratch (part_bytes + part2_bytes) on `st`; dout receives 32*rows bytes
// (encode) or, with encode = false, 128*rows bytes of extended points. sums_extra: 128*rows bytes for the row sums, or null
static void msm_enqueue_reduce(sp_ctx* c, hipStream_t st, const MsmPlan& m, size_t rows, uint8_t* scratch, uint8_t* dout, bool encode,
                               uint8_t* sums_extra, const unsigned* qcounts) {
  Pt* partial = (Pt*)scratch;
  Pt10* partial2 = (Pt10*)(scratch + m.part_bytes);
  // many rows: sums first, then one lane per row encodes (k_pt_encode). The sums reuse the head of the partial buffer of
  // the pass that has already been consumed: two-pass -> `partial`, one-pass -> needs rows*128 B <= part2... so one-pass
  // shapes keep them behind the partials (the caller's scratch has 32*rows spare there only when sums_extra is set)
  const bool batch_encode = encode && rows >= 64 && sums_extra != nullptr;
  const bool encode_in_reduce = encode && !batch_encode;
  Pt* sums = (Pt*)sums_extra;
  uint8_t* dst = batch_encode ? (uint8_t*)sums : dout;
  auto scope = [&](int fam, double bytes) { return ProfScope(c, fam, bytes, st); };  // HIP events on the stream the kernels run on
  if (m.two_pass) {
    {
      ProfScope ps = scope(PF_MSM_REDUCE_PASS, (double)(rows * m.P * sizeof(Pt)) + (double)(rows * m.nchunks * sizeof(Pt10)));
      hipLaunchKernelGGL(k_pt_reduce_pass, dim3((unsigned)rows, (unsigned)m.nchunks), dim3(256), 0, st, (const Pt*)partial, m.P, m.chunk, partial2, qcounts);
    }
    ProfScope ps = scope(PF_MSM_REDUCE, (double)(rows * m.nchunks * sizeof(Pt10)) + 32.0 * (double)rows);
    auto reduce = encode_in_reduce ? k_msm_reduce<true, true> : k_msm_reduce<true, false>;
    hipLaunchKernelGGL(reduce, dim3((unsigned)rows), dim3(256), 0, st, (const void*)partial2, m.nchunks, dst, (const unsigned*)nullptr);
  } else {
    ProfScope ps = scope(PF_MSM_REDUCE, (double)(rows * m.P * sizeof(Pt)) + 32.0 * (double)rows);
    auto reduce = encode_in_reduce ? k_msm_reduce<false, true> : k_msm_reduce<false, false>;
    hipLaunchKernelGGL(reduce, dim3((unsigned)rows), dim3(256), 0, st, (const void*)partial, m.P, dst, qcounts);
  }
  if (batch_encode) {
    ProfScope ps = scope(PF_MSM_REDUCE, 160.0 * (double)rows);
    // (the background launch of a co-resident pair encodes under the other launch: the variant that fits next to it)
    if (m.queue && m.qrole == MSMQ_CORESIDENT && st != c->stream)
      hipLaunchKernelGGL(k_pt_encode_lean, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, (const Pt*)sums, rows, dout);
    else
      hipLaunchKernelGGL(k_pt_encode, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, (const Pt*)sums, rows, dout);
  }
}
// one many-row commit on `st`: the sums, then the reduction with the batch encode, in `scratch` (layout lay); the encodings go to dout
static void msm_enqueue_commit(sp_ctx* c, hipStream_t st, const MsmPlan& m, const MsmScratch& lay, const sp_gens* g, const Fq* dZ, size_t z_stride, size_t rows,
                               size_t cols, size_t g_off, const uint32_t* didx, const Fq* dblinds, size_t h_idx, uint8_t* scratch, uint8_t* dout) {
  const unsigned* qcounts = msm_enqueue_sums(c, st, m, g, dZ, z_stride, rows, cols, g_off, didx, dblinds, h_idx, scratch);
  msm_enqueue_reduce(c, st, m, rows, scratch, dout, true, scratch + lay.sums_off, qcounts);
}
// the one-block tree on `st`: the sum of each row (at most 256 (column, window) pairs) as a point at sums_out. The caller holds the profile scope
static void msm_tree1_enqueue(hipStream_t st, const sp_gens* g, const Fq* dZ, size_t z_stride, size_t rows, size_t cols, size_t g_off, const uint32_t* didx,
                              size_t idx_row_stride, const Fq* dblinds, size_t h_idx, uint8_t* sums_out) {
  hipLaunchKernelGGL((k_msm_windows_tree<true>), dim3(1, (unsigned)rows), dim3(256), 0, st, dZ, z_stride, cols, (const Niels*)g->table, g_off, didx, idx_row_stride,
                     dblinds, h_idx, (void*)sums_out, g->geom);
}
// the ending of a few-row commit: the row sums lie at `sums` (the host-mapped page; device memory when the plan encodes on the device) and go out as
// points, as host-core encodings or through k_pt_encode. waited: the launch that wrote them has already been waited for (the fused tree's flag)
static int32_t msm_finish_few(sp_ctx* c, const MsmPlan& m, size_t rows, const uint8_t* sums, bool waited, uint8_t* out_host, Pt* points_out) {
  if (m.encode_dev) {
    {
      ProfScope ps(c, PF_MSM_REDUCE, 160.0 * (double)rows);
      hipLaunchKernelGGL(k_pt_encode, dim3(1), dim3(64), 0, c->stream, (const Pt*)sums, rows, hres(c));
    }
    SPCHK(fetch_small(c, out_host, 32 * rows));
    return hipGetLastError() == hipSuccess ? SP_OK : SP_EHIP;
  }
  if (!waited) SPCHK(sync_spin(c));
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  Pt pts[SP_HOST_ENCODE_ROWS];  // out of the host-mapped page first: the encodes read each coordinate several times
  memcpy(pts, sums, sizeof(Pt) * rows);
  if (points_out) memcpy(points_out, pts, sizeof(Pt) * rows);
  else pt_compress_many(pts, rows, out_host);
  return SP_OK;
}
// core: Z on device (row stride in elements), optional idx (device), optional blinds (device); synchronous
int32_t msm_launch(sp_ctx* c, const sp_gens* g, const Fq* dZ, size_t z_stride, size_t rows, size_t cols, size_t g_off,
                   const uint32_t* didx, const Fq* dblinds, size_t h_idx, uint8_t* out_host, size_t idx_row_stride, Pt* points_out) {
  if (idx_row_stride && (!didx || rows > SP_HOST_ENCODE_ROWS)) return SP_EINVAL;
  if (points_out && (rows > SP_HOST_ENCODE_ROWS || c->device_encode)) return SP_EINVAL;  // row sums as points: the few-row path only
  MsmPlan m = msm_plan(c, g, rows, cols, dblinds != nullptr, 0, 0, c->bg_inflight > 0);
  const MsmScratch lay = msm_scratch(m, rows);
  SPCHK(ensure(&c->scratch, &c->scratch_cap, lay.bytes));
  uint8_t* const scratch = (uint8_t*)c->scratch;
  if (!m.few) {
    bool small_out = 32 * rows <= HMAP_SIZE - HMAP_IN;
    uint8_t* dout = small_out ? hres(c) : scratch + lay.out_off;
    msm_enqueue_commit(c, c->stream, m, lay, g, dZ, z_stride, rows, cols, g_off, didx, dblinds, h_idx, scratch, dout);
    if (small_out) SPCHK(fetch_small(c, out_host, 32 * rows));
    else SPCHK(fetch_out(c, dout, out_host, 32 * rows));
    return hipGetLastError() == hipSuccess ? SP_OK : SP_EHIP;
  }
  uint8_t* sums_dst = m.encode_dev ? scratch + lay.sums_off : hres(c);
  if (m.tree == MSM_TREE_NONE) {
    if (idx_row_stride) {  // per-row index lists exist on the lookup+tree path only: longer rows go out one at a time, each with its own list
      for (size_t r = 0; r < rows; r++)  // (an inner-product round of more than 2^19 lookups that is not fusable: n0 = 32768, or 16384 at narrow windows)
        SPCHK(msm_launch(c, g, dZ + r * z_stride, z_stride, 1, cols, g_off, didx + r * idx_row_stride, dblinds ? dblinds + r : nullptr, h_idx,
                         out_host ? out_host + 32 * r : nullptr, 0, points_out ? points_out + r : nullptr));
      return SP_OK;
    }
    const unsigned* qcounts = msm_enqueue_sums(c, c->stream, m, g, dZ, z_stride, rows, cols, g_off, didx, dblinds, h_idx, scratch);
    msm_enqueue_reduce(c, c->stream, m, rows, scratch, sums_dst, false, nullptr, qcounts);
    return msm_finish_few(c, m, rows, sums_dst, false, out_host, points_out);
  }
  Pt10* part = (Pt10*)scratch;
  const DoneSig sig = m.tree == MSM_TREE_FUSED ? sig_make(c, m.nblk * rows) : sig_none();
  {
    ProfScope ps(c, PF_MSM_WINDOWS, 32.0 * (double)(rows * cols) + 160.0 * (double)(rows * m.nblk));
    if (m.tree == MSM_TREE1)
      msm_tree1_enqueue(c->stream, g, dZ, z_stride, rows, cols, g_off, didx, idx_row_stride, dblinds, h_idx, sums_dst);
    else if (m.tree == MSM_TREE_FUSED)
      hipLaunchKernelGGL(k_msm_windows_tree_fused, dim3((unsigned)m.nblk, (unsigned)rows), dim3(256), 0, c->stream, dZ, z_stride, cols, (const Niels*)g->table, g_off,
                         didx, idx_row_stride, dblinds, h_idx, part, c->done_counter + 4, (Pt*)sums_dst, g->geom, sig);
    else
      hipLaunchKernelGGL((k_msm_windows_tree<false>), dim3((unsigned)m.nblk, (unsigned)rows), dim3(256), 0, c->stream, dZ, z_stride, cols,
                         (const Niels*)g->table, g_off, didx, idx_row_stride, dblinds, h_idx, (void*)part, g->geom);
  }
  if (m.tree == MSM_TREE_FUSED) SPCHK(sig_wait(c, sig));
  if (m.tree == MSM_TREE_UNFUSED) {
    ProfScope ps(c, PF_MSM_REDUCE, 160.0 * (double)(rows * m.nblk) + 128.0 * (double)rows);
    hipLaunchKernelGGL((k_msm_reduce<true, false>), dim3((unsigned)rows), dim3(256), 0, c->stream, (const void*)part, m.nblk, sums_dst, (const unsigned*)nullptr);
  }
  return msm_finish_few(c, m, rows, sums_dst, m.tree == MSM_TREE_FUSED, out_host, points_out);
}

extern "C" {
// the argument check of the table-based entry points: a rows x cols matrix at Z[z_off..] (rows z_stride apart) against the generators
// [g_off, g_off + cols) and, with blinds, generator h_idx; `out` is the entry point's result pointer
static bool commit_args_ok(const sp_ctx* c, const sp_gens* g, const sp_table* Z, const void* out, size_t g_off, size_t h_idx, bool blinds, size_t z_off,
                           size_t z_stride, size_t rows, size_t cols) {
  return c && g && Z && out && rows != 0 && cols != 0 && z_stride >= cols && g_off + cols <= g->n && (!blinds || h_idx < g->n) &&
         z_off + (rows - 1) * z_stride + cols <= Z->cap;
}
// host blinds -> the device staging buffer (async on the main stream); *dbl = null when there are none
static int32_t stage_blinds(sp_ctx* c, const uint64_t* blinds, size_t rows, const Fq** dbl) {
  *dbl = nullptr;
  if (!blinds) return SP_OK;
  SPCHK(ensure_dstage(c, 32 * rows));
  SPCHK(stage_in(c, 0, blinds, 32 * rows));
  *dbl = (const Fq*)c->dstage;
  return SP_OK;
}
// open a job for plan m on `st`: the sp_job, its scratch from the pool (layout: msm_scratch) and its `done` event
static int32_t job_open(sp_ctx* c, hipStream_t st, const MsmPlan& m, size_t rows, sp_job** out, MsmScratch* lay) {
  sp_job* j = new (std::nothrow) sp_job();
  if (!j) return SP_ENOMEM;
  *lay = msm_scratch(m, rows);
  j->ctx = c; j->rows = rows; j->scratch = nullptr; j->stream = st;
  j->out_off = lay->out_off;
  j->scratch_bytes = lay->bytes;
  int32_t rc = pool_alloc(c, j->scratch_bytes, (void**)&j->scratch);
  if (rc != SP_OK) { delete j; return rc; }
  if (hipEventCreateWithFlags(&j->done, hipEventDisableTiming) != hipSuccess) { pool_release(c, j->scratch, j->scratch_bytes); delete j; return SP_EHIP; }
  *out = j;
  return SP_OK;
}
// abandon a job that was opened and will not be handed out
static void job_abandon(sp_job* j) {
  (void)hipEventDestroy(j->done);
  pool_release(j->ctx, j->scratch, j->scratch_bytes);
  delete j;
}

// ---- background commit (overlaps a throughput-bound MSM with the latency-bound rounds that follow on the main stream)
int32_t sp_commit_rows_dev_begin(sp_ctx* c, const sp_gens* g, size_t g_off, const sp_table* Z, size_t z_off, size_t rows, size_t cols,
                                 sp_job** out) {
  if (!commit_args_ok(c, g, Z, out, g_off, 0, false, z_off, cols, rows, cols)) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  MsmPlan m = msm_plan(c, g, rows, cols, false, c->bg_blocks > 0 ? (size_t)c->bg_blocks * 4 : 0);
  sp_job* j = nullptr;
  MsmScratch lay;
  SPCHK(job_open(c, c->stream_bg, m, rows, &j, &lay));
  hipEvent_t ready;
  if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess) { job_abandon(j); return SP_EHIP; }
  // the job reads Z as produced by everything queued so far on the main stream
  (void)hipEventRecord(ready, c->stream);
  (void)hipStreamWaitEvent(c->stream_bg, ready, 0);
  msm_enqueue_commit(c, c->stream_bg, m, lay, g, Z->d + z_off, cols, rows, cols, g_off, nullptr, nullptr, 0, j->scratch, j->scratch + lay.out_off);
  (void)hipEventRecord(j->done, c->stream_bg);
  (void)hipEventDestroy(ready);
  if (hipGetLastError() != hipSuccess) { job_abandon(j); return SP_EHIP; }
  c->bg_inflight++;
  *out = j;
  return SP_OK;
}
// Foreground variant: the commit (with blinds) is queued on the MAIN stream at full width and the call returns; the caller
// may do host work (it must not make another call on this context) until sp_job_wait. Used to hash the computation
// commitment into the transcript (0.65 ms of Keccak at 2^20) while the witness commitment is being computed.
int32_t sp_commit_rows_dev_start(sp_ctx* c, const sp_gens* g, size_t g_off, size_t h_idx, const sp_table* Z, size_t z_off, size_t rows, size_t cols,
                                 const uint64_t* blinds, sp_job** out) {
  if (!commit_args_ok(c, g, Z, out, g_off, h_idx, blinds != nullptr, z_off, cols, rows, cols) || rows <= SP_HOST_ENCODE_ROWS) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const Fq* dbl = nullptr;
  SPCHK(stage_blinds(c, blinds, rows, &dbl));
  MsmPlan m = msm_plan(c, g, rows, cols, blinds != nullptr, 0, 0, c->bg_inflight > 0);
  sp_job* j = nullptr;
  MsmScratch lay;
  SPCHK(job_open(c, c->stream, m, rows, &j, &lay));
  msm_enqueue_commit(c, c->stream, m, lay, g, Z->d + z_off, cols, rows, cols, g_off, nullptr, dbl, h_idx, j->scratch, j->scratch + lay.out_off);
  (void)hipEventRecord(j->done, c->stream);
  if (hipGetLastError() != hipSuccess) { job_abandon(j); return SP_EHIP; }
  *out = j;
  return SP_OK;
}
// The same commit with the rows still in HOST memory (the satisfying assignment SNARK::prove is handed: src/lib.rs:339-344): the rows
// are copied into Z[z_off..] in four chunks and the MSM of a chunk is launched behind its copy, so the additions of chunk k run while
// chunk k + 1 crosses PCIe (32 MB at 2^20: 0.65 ms of copy, 0.87 ms of MSM); one reduction + encode over all rows at the end.
// Collected with sp_job_wait like the other forms. Shapes the chunking does not fit (few rows, rows not a multiple of 1024, the
// lookup form) take copy-then-commit.
int32_t sp_commit_rows_upload_start(sp_ctx* c, const sp_gens* g, size_t g_off, size_t h_idx, sp_table* Z, size_t z_off, const uint64_t* src, size_t rows,
                                    size_t cols, const uint64_t* blinds, sp_job** out) {
  if (!commit_args_ok(c, g, Z, out, g_off, h_idx, blinds != nullptr, z_off, cols, rows, cols) || !src || rows <= SP_HOST_ENCODE_ROWS) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const size_t nch = (size_t)c->opt.v[OPT_UPLOAD_CHUNKS];
  const bool chunked_on = c->opt.v[OPT_UPLOAD_OVERLAP] != 0;  // A/B switch
  MsmPlan m = msm_plan(c, g, rows, cols, blinds != nullptr, 0, chunked_on && rows % (256 * nch) == 0 ? rows / nch : 0, c->bg_inflight > 0);
  if (!chunked_on || m.windowed || rows % (256 * nch) != 0) {
    HIPCHK(hipMemcpyAsync(Z->d + z_off, src, 32 * rows * cols, hipMemcpyHostToDevice, c->stream));
    return sp_commit_rows_dev_start(c, g, g_off, h_idx, Z, z_off, rows, cols, blinds, out);
  }
  const Fq* dbl = nullptr;
  SPCHK(stage_blinds(c, blinds, rows, &dbl));
  sp_job* j = nullptr;
  MsmScratch lay;
  SPCHK(job_open(c, c->stream, m, rows, &j, &lay));
  const size_t rch = rows / nch;
  const unsigned* qcounts = nullptr;
  // copies on the side stream, back to back; the additions of a chunk on the main stream, behind that chunk's copy
  hipEvent_t ready = nullptr;
  hipError_t e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(ready, c->stream);  // Z as left by what the main stream has queued (its zero fill)
  if (e == hipSuccess) e = hipStreamWaitEvent(c->stream_side, ready, 0);
  if (ready) (void)hipEventDestroy(ready);
  for (size_t k = 0; k < nch && e == hipSuccess; k++) {
    const size_t r0 = k * rch;
    // (a copy from pageable memory returns when the data has left the host buffer)
    e = hipMemcpyAsync(Z->d + z_off + r0 * cols, src + 4 * r0 * cols, 32 * rch * cols, hipMemcpyHostToDevice, c->stream_side);
    hipEvent_t copied = nullptr;  // one event per chunk (an event re-recorded while a wait on it is pending is not something to rely on)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&copied, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(copied, c->stream_side);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, copied, 0);
    if (copied) (void)hipEventDestroy(copied);
    if (e == hipSuccess)
      qcounts = msm_enqueue_sums(c, c->stream, m, g, Z->d + z_off + r0 * cols, cols, rch, cols, g_off, nullptr, dbl ? dbl + r0 : nullptr, h_idx,
                                 j->scratch + r0 * m.P * sizeof(Pt));
  }
  // The queue form is planned only for an upload issued as ONE chunk (launch_rows == rows, upload.chunks = 1): its slot counts then cover every
  // row, and the reduction must have them — a slot no wavefront attached to holds no sum. (Without them every row of such a commit came out wrong.)
  // The other forms return none.
  if (e == hipSuccess) msm_enqueue_reduce(c, c->stream, m, rows, j->scratch, j->scratch + lay.out_off, true, j->scratch + lay.sums_off, nch == 1 ? qcounts : nullptr);
  (void)hipEventRecord(j->done, c->stream);
  if (e != hipSuccess || hipGetLastError() != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    job_abandon(j);
    return SP_EHIP;
  }
  *out = j;
  return SP_OK;
}
int32_t sp_job_wait(sp_job* j, uint8_t* out) {
  if (!j || !out) return SP_EINVAL;
  sp_ctx* c = j->ctx;
  HIPCHK(hipSetDevice(c->dev));
  int32_t rc = SP_OK;
  for (;;) {
    hipError_t e = hipEventQuery(j->done);
    if (e == hipSuccess) break;
    if (e != hipErrorNotReady) { rc = SP_EHIP; break; }
  }
  if (rc == SP_OK) {
    if (hipMemcpyAsync(out, j->scratch + j->out_off, 32 * j->rows, hipMemcpyDeviceToHost, j->stream) != hipSuccess ||
        hipStreamSynchronize(j->stream) != hipSuccess)
      rc = SP_EHIP;
  }
  if (j->stream == c->stream_bg && c->bg_inflight > 0) c->bg_inflight--;
  // the scratch goes back to the pool, which hands it to main-stream work: make that work wait for the job
  (void)hipStreamWaitEvent(c->stream, j->done, 0);
  (void)hipEventDestroy(j->done);
  pool_release(c, j->scratch, j->scratch_bytes);
  delete j;
  return rc;
}

int32_t sp_commit_rows_dev(sp_ctx* c, const sp_gens* g, size_t g_off, size_t h_idx, const sp_table* Z, size_t z_off, size_t rows, size_t cols,
                           const uint64_t* blinds, uint8_t* out) {
  if (!commit_args_ok(c, g, Z, out, g_off, h_idx, blinds != nullptr, z_off, cols, rows, cols)) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const Fq* dbl = nullptr;
  SPCHK(stage_blinds(c, blinds, rows, &dbl));
  return msm_launch(c, g, Z->d + z_off, cols, rows, cols, g_off, nullptr, dbl, h_idx, out);
}
// A commitment restricted to a run of generators, left as points: sum_j Z[r * z_stride + j] * G[g_off + j], j < cols, for rows <= 8, no
// blind. The building block of a COLUMN-sharded commitment (the north-star's partial sums): every shard sums its slice of
// the generators, the W partial points of a row are gathered and added (sp_host_points_sum_encode) — the only way to shard a commitment
// with fewer rows than shards (Cx of DotProductProofLog, a small instance's witness).
int32_t sp_commit_rows_partial(sp_ctx* c, const sp_gens* g, size_t g_off, const sp_table* Z, size_t z_off, size_t z_stride, size_t rows, size_t cols,
                               sp_host_point* out) {
  if (!commit_args_ok(c, g, Z, out, g_off, 0, false, z_off, z_stride, rows, cols) || rows > SP_HOST_ENCODE_ROWS) return SP_EINVAL;
  static_assert(sizeof(sp_host_point) == sizeof(Pt), "sp_host_point carries an extended point");
  HIPCHK(hipSetDevice(c->dev));
  return msm_launch(c, g, Z->d + z_off, z_stride, rows, cols, g_off, nullptr, nullptr, 0, nullptr, 0, (Pt*)out);
}
int32_t sp_commit_rows(sp_ctx* c, const sp_gens* g, size_t g_off, size_t h_idx, const uint64_t* Z, size_t rows, size_t cols,
                       const uint64_t* blinds, uint8_t* out) {
  if (!c || !g || !Z || !out || rows == 0 || cols == 0) return SP_EINVAL;
  if (g_off + cols > g->n || (blinds && h_idx >= g->n)) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  size_t zb = 32 * rows * cols;
  HIPCHK(hipStreamSynchronize(c->stream));
  SPCHK(ensure(&c->scratch2, &c->scratch2_cap, zb + 32 * rows));
  HIPCHK(hipMemcpyAsync(c->scratch2, Z, zb, hipMemcpyHostToDevice, c->stream));
  const Fq* dbl = nullptr;
  if (blinds) {
    HIPCHK(hipMemcpyAsync((uint8_t*)c->scratch2 + zb, blinds, 32 * rows, hipMemcpyHostToDevice, c->stream));
    dbl = (const Fq*)((uint8_t*)c->scratch2 + zb);
  }
  return msm_launch(c, g, (const Fq*)c->scratch2, cols, rows, cols, g_off, nullptr, dbl, h_idx, out);
}
static bool idx_in_set(const sp_gens* g, const uint32_t* idx, size_t cols) {
  for (size_t j = 0; j < cols; j++)
    if (idx[j] >= g->n) return false;
  return true;
}
// rows x cols scalars and one index list, staged where the kernel reads them: *ds, *di. page_only: refused when they do not fit the page
static int32_t stage_indexed(sp_ctx* c, const uint32_t* idx, size_t cols, const uint64_t* S, size_t rows, bool page_only, const Fq** ds, const uint32_t** di) {
  size_t sb = 32 * rows * cols, ib = (4 * cols + 31) & ~(size_t)31;
  if (sb + ib <= HMAP_GEN) {  // Sigma-protocol sized: the kernel reads scalars and indices straight from the host-mapped page
    *ds = (const Fq*)stage_small(c, 0, S, sb);
    *di = (const uint32_t*)stage_small(c, sb, idx, 4 * cols);
    return SP_OK;
  }
  if (page_only) return SP_EINVAL;
  SPCHK(ensure_dstage(c, sb + ib));
  SPCHK(stage_in(c, 0, S, sb));
  SPCHK(stage_in(c, sb, idx, 4 * cols));
  *ds = (const Fq*)c->dstage;
  *di = (const uint32_t*)((uint8_t*)c->dstage + sb);
  return SP_OK;
}
int32_t msm_small_enqueue(sp_ctx* c, hipStream_t st, const sp_gens* g, const uint32_t* idx, size_t cols, const uint64_t* S, size_t rows,
                          uint8_t* sums_out) {
  if (!c || !g || !idx || !S || !sums_out || rows == 0 || rows > SP_HOST_ENCODE_ROWS || cols == 0 || cols * (size_t)g->geom.nwin > 256) return SP_EINVAL;
  if (!idx_in_set(g, idx, cols)) return SP_EINVAL;
  const Fq* ds = nullptr;
  const uint32_t* di = nullptr;
  SPCHK(stage_indexed(c, idx, cols, S, rows, true, &ds, &di));
  ProfScope ps(c, PF_MSM_WINDOWS, 32.0 * (double)(rows * cols) + 128.0 * (double)rows, st);
  msm_tree1_enqueue(st, g, ds, cols, rows, cols, 0, di, 0, nullptr, 0, sums_out);
  return SP_OK;
}
int32_t sp_msm_indexed(sp_ctx* c, const sp_gens* g, const uint32_t* idx, size_t cols, const uint64_t* S, size_t rows, uint8_t* out) {
  if (!c || !g || !idx || !S || !out || rows == 0 || cols == 0 || !idx_in_set(g, idx, cols)) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const Fq* ds = nullptr;
  const uint32_t* di = nullptr;
  SPCHK(stage_indexed(c, idx, cols, S, rows, false, &ds, &di));
  return msm_launch(c, g, ds, cols, rows, cols, 0, di, nullptr, 0, out);
}
}  // extern "C"
