// spartan_amd: the gathered wide-window forms of the fixed-base row MSM: strip, background and balanced kernels, the one-lookup-per-thread form.
#include "internal.hpp"
#include <mutex>

// thread <-> (row, strip): accumulates sum_{j in strip} Z[row][j] * P[col(j)] into one extended point.
// Lanes run fastest over rows so a wave shares the generator (and its 12 KiB window sub-table) whenever
// rows >= 64: table gathers then hit L1/L2, while the scalar load (32 B per 32 additions) is the strided one.
template <bool PF2>
__device__ __forceinline__ void msm_rows_tile(size_t lb, unsigned tid, const Fq* __restrict__ Z, size_t z_row_stride, size_t rows, size_t cols,
                                              size_t strip, size_t nstrips, const Niels* __restrict__ table, size_t g_off,
                                              const uint32_t* __restrict__ idx, const Fq* __restrict__ blinds, size_t h_idx, Pt* __restrict__ partial,
                                              int xcd_map, const MsmGeom& geom) {
  size_t row, s;
  if (xcd_map) {
    // XCD-aware tile order (block b runs on XCD b % 8, each XCD has its own L2): all row-blocks of a column strip are
    // given to the SAME XCD, back to back, so the strip's window tables are fetched into one L2 instead of eight.
    size_t rb_count = rows / 256, xcd = lb % 8, k = lb / 8;
    s = xcd + 8 * (k / rb_count);
    if (s >= nstrips) return;
    row = (k % rb_count) * 256 + tid;
  } else {
    size_t t = lb * 256 + tid;
    if (t >= rows * nstrips) return;
    row = t % rows;
    s = t / rows;
  }
  Pt acc = pt_identity();
  size_t j0 = s * strip, j1 = j0 + strip;
  if (j1 > cols) j1 = cols;
  for (size_t j = j0; j < j1; j++) {
    Fq sc = ld_fq(Z + row * z_row_stride + j);
    size_t pt = idx ? (size_t)idx[j] : g_off + j;
    msm_accumulate_t<PF2>(acc, sc, table, pt, geom);
  }
  if (blinds && s == 0) msm_accumulate_t<PF2>(acc, ld_fq(blinds + row), table, h_idx, geom);
  partial[row * nstrips + s] = acc;
}
template <bool PF2>
__global__ void __launch_bounds__(256) k_msm_rows(const Fq* __restrict__ Z, size_t z_row_stride, size_t rows, size_t cols, size_t strip,
                                                  size_t nstrips, const Niels* __restrict__ table, size_t g_off,
                                                  const uint32_t* __restrict__ idx, const Fq* __restrict__ blinds, size_t h_idx,
                                                  Pt* __restrict__ partial, int xcd_map, MsmGeom geom) {
  msm_rows_tile<PF2>(blockIdx.x, threadIdx.x, Z, z_row_stride, rows, cols, strip, nstrips, table, g_off, idx, blinds, h_idx, partial, xcd_map, geom);
}
// Background form: persistent 1024-thread workgroups, launched on fewer workgroups than the chip has CUs. At 127 VGPRs a
// CU holds exactly one of them (16 waves, 508 of 512 registers per lane), so the CUs left over cannot receive a second
// MSM workgroup and the main stream keeps a reserve of idle CUs for its latency-bound kernels — the partition a CU mask
// would give, which this platform does not honour.
__global__ void __launch_bounds__(1024) k_msm_rows_bg(const Fq* __restrict__ Z, size_t z_row_stride, size_t rows, size_t cols, size_t strip,
                                                      size_t nstrips, const Niels* __restrict__ table, size_t g_off, Pt* __restrict__ partial,
                                                      int xcd_map, size_t ntiles, MsmGeom geom) {
  extern __shared__ uint8_t occupancy_fence[];
  for (size_t lb = (size_t)blockIdx.x * 4 + threadIdx.x / 256; lb < ntiles; lb += (size_t)gridDim.x * 4)
    msm_rows_tile<false>(lb, threadIdx.x % 256, Z, z_row_stride, rows, cols, strip, nstrips, table, g_off, nullptr, nullptr, 0, partial, xcd_map, geom);
}
// ---- balanced form of the row MSM (round 4) -----------------------------------------------------------------------------------
// The strip form above gives a thread a whole number of SCALARS, and the launch a number of workgroups that has nothing to do with the
// number the chip holds (3 per CU at 164 VGPRs = 768): a 256 x 1024 witness chunk is 1024 workgroups = 1.33 waves of workgroups (the
// second one a third full: 0.61 of the addition ceiling), the derefs column half 1248 active ones = 1.6 (0.59). Here the unit of work is
// one (column, window) pair = ONE table lookup + ONE mixed addition: a row's cols x nwin units are cut into nb equal runs, run k of
// row-block r is one workgroup, and nb is chosen so that the whole launch is (at most) as many workgroups as the chip holds at once —
// every CU works from the first to the last cycle of the launch and all finish together. A run starts and ends in the middle of a
// scalar: the signed recoding's carry into its first window is rebuilt from the lower windows (integer work, once per thread).
// The digit stream runs seamlessly from one scalar into the next, so the two table entries in flight stay in flight across scalars
// (the strip form drained and refilled its pipeline once per scalar). Lanes are still rows of one column: a wave's 64 gathers of a
// step fall into one (point, window) sub-table.
// Short scalars / zero rows (SNARK::encode's address and timestamp vectors, padding rows): when no lane of the wave has a non-zero
// digit left in the current scalar (ballot), the stream jumps to the next scalar without issuing the remaining gathers.
struct MsmFlatArgs {
  const Fq* Z; size_t z_row_stride, rows, cols;
  const Niels* table; size_t g_off; const uint32_t* idx; const Fq* blinds; size_t h_idx;
  Pt* partial;          // [rows][nb]
  unsigned nb, rb_count;  // runs per row; row-blocks of 256 rows
  MsmGeom geom;
};
struct MsmUnit { const MsmEntry* p; bool neg, nz, valid; };
template <bool AHEAD>  // AHEAD: the next scalar is requested one scalar ahead (8 registers; the 128-register background form does without)
struct MsmDigitStream {
  const MsmFlatArgs& A;
  const size_t row;
  size_t j, ncol;      // current column (wave-uniform); columns incl. the blind
  long left;           // units still to hand out (wave-uniform)
  int w;               // next window of the current scalar (wave-uniform)
  uint64_t s0, s1, s2, s3;  // the current scalar, canonical, shifted down by w windows
  int carry;
  Fq raw_next;         // Montgomery form of column j + 1, requested one scalar ahead
  const MsmEntry* base;
  __device__ __forceinline__ MsmDigitStream(const MsmFlatArgs& A_, size_t row_) : A(A_), row(row_) {}
  __device__ __forceinline__ const Fq* scalar_ptr(size_t jj) const { return jj < A.cols ? A.Z + row * A.z_row_stride + jj : A.blinds + row; }
  __device__ __forceinline__ void set_base(size_t jj) {
    size_t pt = jj < A.cols ? (A.idx ? (size_t)A.idx[jj] : A.g_off + jj) : A.h_idx;
    base = reinterpret_cast<const MsmEntry*>(A.table) + pt * A.geom.pt_entries;
  }
  __device__ __forceinline__ void take(const Fq& raw) {
    Fq s = fq_from_mont(raw);  // canonical integer < q < 2^253 (scalar/mod.rs:32-36 does the same for dalek)
    s0 = s.l[0]; s1 = s.l[1]; s2 = s.l[2]; s3 = s.l[3];
    carry = 0;
  }
  __device__ __forceinline__ void shift(int c) {
    s0 = (s0 >> c) | (s1 << (64 - c));
    s1 = (s1 >> c) | (s2 << (64 - c));
    s2 = (s2 >> c) | (s3 << (64 - c));
    s3 >>= c;
  }
  __device__ __forceinline__ void open(size_t u0, size_t u1) {
    const int nwin = A.geom.nwin;
    ncol = A.cols + (A.blinds ? 1 : 0);
    left = (long)(u1 - u0);
    j = u0 / (size_t)nwin;
    w = (int)(u0 % (size_t)nwin);
    if (left <= 0) { left = 0; base = reinterpret_cast<const MsmEntry*>(A.table); s0 = s1 = s2 = s3 = 0; carry = 0; raw_next = fq_zero(); return; }
    take(ld_fq(scalar_ptr(j)));
    set_base(j);
    if (AHEAD) raw_next = j + 1 < ncol ? ld_fq(scalar_ptr(j + 1)) : fq_zero();
    for (int k = 0; k < w; k++) {  // the carry into window w depends on all lower windows
      const int c = msm_wbits_of(A.geom, k);
      int d = (int)(s0 & ((1u << c) - 1)) + carry;
      carry = d >= (1 << (c - 1));
      shift(c);
    }
  }
  __device__ __forceinline__ void next(MsmUnit& u) {
    const int nwin = A.geom.nwin;
    for (;;) {
      if (left == 0) { u.p = base; u.neg = false; u.nz = false; u.valid = false; return; }
      if (w == nwin) {
        j++;
        if (AHEAD) {
          take(raw_next);
          raw_next = j + 1 < ncol ? ld_fq(scalar_ptr(j + 1)) : fq_zero();
        } else {
          take(ld_fq(scalar_ptr(j)));
        }
        set_base(j);
        w = 0;
      }
      if (__all((s0 | s1 | s2 | s3) == 0 && carry == 0)) {  // nothing left in this scalar on any lane of the wave: no gathers for its upper windows
        long k = nwin - w;
        if (k > left) k = left;
        left -= k;
        w = nwin;
        continue;
      }
      break;
    }
    const int c = msm_wbits_of(A.geom, w);
    int d = (int)(s0 & ((1u << c) - 1)) + carry;
    carry = d >= (1 << (c - 1));
    d -= carry << c;
    uint32_t m = (uint32_t)(d < 0 ? -d : d);
    u.p = base + msm_woff(A.geom, w) + (m ? m - 1 : 0);
    u.neg = d < 0; u.nz = m != 0; u.valid = true;
    shift(c);
    w++; left--;
  }
};
// Two entries in flight, each for the time of two additions: the loop is unrolled twice so that the registers of an entry in flight are never
// the source of a copy — the compiler's waits then allow the 12 most recent loads to stay outstanding. (The rolled form with the second
// entry copied each step, and the one-entry form of a 128-register background variant, were measured in round 4 and retired in round 6.)
__device__ __forceinline__ void msm_flat_tile(const MsmFlatArgs& A, unsigned lb, unsigned tid) {
  const unsigned rb = lb % A.rb_count, bk = lb / A.rb_count;
  if (bk >= A.nb) return;
  const size_t row = (size_t)rb * 256 + tid;
  const size_t U = (A.cols + (A.blinds ? 1 : 0)) * (size_t)A.geom.nwin;
  const size_t u0 = U * bk / A.nb, u1 = U * (bk + 1) / A.nb;
  Pt acc = pt_identity();
  MsmDigitStream<true> ds(A, row);
  ds.open(u0, u1);
  MsmUnit a;
  ds.next(a);
  MsmEntry X = msm_load(a.p);
  MsmUnit b;
  ds.next(b);
  MsmEntry Y = msm_load(b.p);
#pragma unroll 1
  while (a.valid) {
    MsmEntry cur = X;
    MsmUnit ca = a;
    ds.next(a);
    X = msm_load(a.p);
    if (ca.nz) acc = pt_madd(acc, msm_entry_niels(cur), ca.neg);
    if (!b.valid) break;
    cur = Y;
    ca = b;
    ds.next(b);
    Y = msm_load(b.p);
    if (ca.nz) acc = pt_madd(acc, msm_entry_niels(cur), ca.neg);
  }
  A.partial[row * A.nb + bk] = acc;
}
__global__ void __launch_bounds__(256) k_msm_flat(MsmFlatArgs A) { msm_flat_tile(A, blockIdx.x, threadIdx.x); }

// Latency-bound shapes (Sigma-protocol commits, IPA rounds, single-row commits): one thread per (row, column,
// window) performs a single table lookup, so the serial chain per thread is one mixed addition instead of 32.
// partial[row][w*cols + j].  The blind, if any, is column `cols` (generator h_idx).
__global__ void __launch_bounds__(256) k_msm_windows(const Fq* __restrict__ Z, size_t z_row_stride, size_t rows, size_t cols,
                                                     const Niels* __restrict__ table, size_t g_off, const uint32_t* __restrict__ idx,
                                                     const Fq* __restrict__ blinds, size_t h_idx, Pt* __restrict__ partial, MsmGeom geom) { SP_FG_PRIO();
  size_t ncol = cols + (blinds ? 1 : 0);
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * ncol * geom.nwin) return;
  size_t row = t % rows, rest = t / rows;
  size_t j = rest % ncol;
  int w = (int)(rest / ncol);
  Fq sc = j < cols ? ld_fq(Z + row * z_row_stride + j) : ld_fq(blinds + row);
  size_t pt = j < cols ? (idx ? (size_t)idx[j] : g_off + j) : h_idx;
  Pt acc = pt_identity();
  if (!fq_is_zero(sc)) {
    Fq s = fq_from_mont(sc);
    int d = msm_digit(s, w, geom);
    if (d != 0) acc = pt_madd(acc, table[msm_tidx(geom, pt, w, d < 0 ? -d : d)], d < 0);
  }
  partial[row * (ncol * geom.nwin) + (size_t)w * ncol + j] = acc;
}
// workgroups of 256 threads the chip holds at once for the balanced row MSM (occupancy of the kernel x CUs), per device
size_t msm_flat_slots() {
  static std::mutex mu;
  static std::map<int, size_t> slots;  // device -> resident workgroups
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 768;
  std::lock_guard<std::mutex> lk(mu);
  auto it = slots.find(dev);
  if (it != slots.end()) return it->second;
  int per_cu = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 768;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_msm_flat, 256, 0);
  if (e != hipSuccess || per_cu < 1) per_cu = 3;
  return slots[dev] = (size_t)per_cu * (size_t)prop.multiProcessorCount;
}
// enqueue of the lookups on `st` (the reduction is the caller's, as for the other forms). MSM_ROWS_WINDOWS: partial[row][P], P = (cols + blind) x
// windows; MSM_ROWS_STRIP: partial[row][P], P = strips of `strip` columns; MSM_ROWS_FLAT: partial[row][P], P = runs per row (rows % 256 == 0)
void msm_rows_enqueue(sp_ctx* c, hipStream_t st, const sp_gens* g, const Fq* dZ, size_t z_stride, size_t rows, size_t cols, size_t g_off,
                      const uint32_t* didx, const Fq* dblinds, size_t h_idx, Pt* partial, int form, size_t strip, size_t P) {
  if (form == MSM_ROWS_WINDOWS) {
    size_t nthreads = rows * P;
    hipLaunchKernelGGL(k_msm_windows, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, dZ, z_stride, rows, cols, (const Niels*)g->table,
                       g_off, didx, dblinds, h_idx, partial, g->geom);
    return;
  }
  if (form == MSM_ROWS_FLAT) {
    MsmFlatArgs A{dZ, z_stride, rows, cols, (const Niels*)g->table, g_off, didx, dblinds, h_idx, partial, (unsigned)P, (unsigned)(rows / 256), g->geom};
    const unsigned ntiles = A.nb * A.rb_count;
    hipLaunchKernelGGL(k_msm_flat, dim3(ntiles), dim3(256), 0, st, A);
    return;
  }
  const size_t nstrips = P;
  int xcd_map = rows % 256 == 0;
  size_t nblocks = xcd_map ? ((nstrips + 7) / 8) * 8 * (rows / 256) : (rows * nstrips + 255) / 256;
  if (st != c->stream && !didx && !dblinds && c->bg_blocks > 0) {
    hipLaunchKernelGGL(k_msm_rows_bg, dim3((unsigned)c->bg_blocks), dim3(1024), (unsigned)c->bg_lds, st, dZ, z_stride, rows, cols, strip, nstrips,
                       (const Niels*)g->table, g_off, partial, xcd_map, nblocks, g->geom);
  } else {
    hipLaunchKernelGGL(k_msm_rows<true>, dim3((unsigned)nblocks), dim3(256), 0, st, dZ, z_stride, rows, cols, strip, nstrips,
                       (const Niels*)g->table, g_off, didx, dblinds, h_idx, partial, xcd_map, g->geom);
  }
}
