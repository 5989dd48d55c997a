// spartan_amd: generators: point decoding, window tables, the process-wide table cache and the geometry policy.
#include "internal.hpp"
#include <algorithm>
#include <list>
#include <mutex>

// stage 1: decode / map points. mode 0: compressed in (32 B); mode 1: uniform in (64 B) -> also writes compressed.
__global__ void k_points_load(const uint8_t* __restrict__ in, int mode, size_t n, Pt* __restrict__ pts, uint8_t* __restrict__ comp_out,
                              int* __restrict__ bad) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Pt p;
  if (mode == 0) {
    uint8_t b[32];
    for (int k = 0; k < 32; k++) b[k] = in[32 * i + k];
    if (!pt_decompress(b, &p)) {
      atomicExch(bad, 1);
      p = pt_identity();
    }
  } else {
    uint8_t b[64];
    for (int k = 0; k < 64; k++) b[k] = in[64 * i + k];
    p = pt_from_uniform_bytes(b);
    if (comp_out) {
      uint8_t c[32];
      pt_compress(p, c);
      for (int k = 0; k < 32; k++) comp_out[32 * i + k] = c[k];
    }
  }
  pts[i] = p;
}
// stage 2: one thread per (point, window, chunk of up to 128 magnitudes): entries k * 2^(c w) * P in affine Niels form.
template <class E>  // E = Niels (one entry per 128-byte line: the gathered wide-window tables) or NielsP (packed: the streamed LDS-form tables)
__global__ void k_table_build(const Pt* __restrict__ pts, size_t n, E* __restrict__ table, MsmGeom geom) {
  // chunks of a point run over its windows in order; a wide window (msm.hpp, mixed widths) is two narrow windows' worth of chunks
  const int chunk = geom.tent < 128 ? geom.tent : 128, nchunk = geom.tent / chunk;
  const size_t per_pt = (size_t)(geom.nwin + geom.nwide) * nchunk;
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * per_pt) return;
  size_t pt = t / per_pt;
  const int slot = (int)((t % per_pt) / nchunk), n0 = msm_n0(geom);   // slot: narrow-window-sized piece of the point's table
  const int w = slot < n0 ? slot : n0 + (slot - n0) / 2;
  int ck = (int)(t % nchunk) + (slot >= n0 && ((slot - n0) & 1) ? nchunk : 0);
  Pt base = pts[pt];
  for (int k = 0; k < msm_bitpos(geom, w); k++) base = pt_dbl(base);
  // first multiple of this chunk: (ck * chunk + 1) * base by double-and-add
  int m0 = ck * chunk + 1;
  Pt acc = pt_identity();
  for (int b = 15; b >= 0; b--) {
    acc = pt_dbl(acc);
    if ((m0 >> b) & 1) acc = pt_add(acc, base);
  }
  for (int m = m0; m < m0 + chunk; m++) {
    Fp zinv = fp_invert(acc.Z);
    Niels e = pt_to_niels(acc, zinv);
    E& dst = table[msm_tidx(geom, pt, w, m)];
    dst.yp = e.yp; dst.ym = e.ym; dst.t2d = e.t2d;
    if (m + 1 < m0 + chunk) acc = pt_add(acc, base);
  }
}

// Window tables are public parameters (MultiCommitGens is immutable, commitments.rs:8-13) and large (7.5 MiB per point):
// they are built once per (device, generator bytes) and shared by every context of the process — concurrent proving
// contexts on one GPU hold one copy, and re-creating a SNARKGens is free. Reference-counted; freed with the last handle.
struct GensCacheEntry {
  int dev, mode;
  MsmGeom geom;
  size_t n, refs;
  std::vector<uint8_t> in, comp;
  Niels* table;
  NielsP* table_lds = nullptr;  // LDS-form tables (msm_lds.hip), built with the set when option msm.lds_bits asks for them — or when the wide tables came out narrow
  int wbits_lds = 0;
  bool prefer_lds = false;
};
static std::mutex g_gens_mu;
static std::list<GensCacheEntry> g_gens_cache;

// Window geometry of a generator set. A committed scalar costs one mixed addition (and one 128-byte gather) per window, so the policy
// minimises the NUMBER of windows under a memory budget; for each number of windows the table is as small as 254 bits allow (mixed
// widths, msm.hpp): per generator 17 windows = 34.6 MB, 18 = 21.0, 19 = 13.6, 20 = 8.9, 21 = 6.0, 22 = 4.5, 24 = 2.5, 26 = 1.5, 32 = 0.5.
//   * 17 windows only while the set's tables stay under msm.wide_gb (default 80: the 1025- and 2049-point streams of a 2^20 / 2^22
//     instance keep them; the proof time of 17 against 18 windows for the larger stream was a tie in rounds 2-4 and costs 56 GB);
//   * otherwise the fewest windows that fit msm.table_gb (default 180 per set: the 8194-point stream of a 2^22 instance at 18 windows is
//     172 GB) and the free device memory less a reserve for the proof's own tables: 24 GB, or 5.0e-7 GB x n^2 when that is more — the
//     working set of a proof grows with the square of its larger generator stream: 134 GB for the 16386 points of a 2^24 instance (instance,
//     encode, proof tables and what the buffer pool keeps: measured on the 309 GB (= 288 GiB) the device reports — with 124 GB left the bench's
//     2^24 run ran out of memory, with 132 it did not);
//     applied only to tables that are themselves large (a 1.5 MB table set must not be refused because another process holds the HBM).
// 2^20: 17 / 18 windows (35.5 + 86.1 GB; rounds 2-5: uniform 15 / 14 bits = 17 / 19 windows, 36.6 + 81.6 GB); 2^22: 17 / 18 (70.9 + 172 GB;
// before 17 / 19, 73 + 163); 2^24: 18 / 22 (86 + 73 GB; before 14 / 12 bits = 19 / 22 windows, 82 + 95). Option msm.windows forces a
// number of windows, msm.wbits a uniform width (the tests use both). Fewer windows than the first choice are reported on stderr (once per
// set): a silent narrowing would be a performance cliff nobody sees. Returns false when not even 32 windows fit in free memory.
static bool choose_geom(const sp_ctx* c, size_t n, MsmGeom* out) {
  if (c->opt.v[OPT_MSM_WBITS] >= 4) { *out = msm_geom((int)c->opt.v[OPT_MSM_WBITS]); return true; }
  if (c->opt.v[OPT_MSM_WINDOWS] >= 17) { *out = msm_geom_windows((int)c->opt.v[OPT_MSM_WINDOWS]); return true; }
  const double budget = (double)c->opt.v[OPT_MSM_TABLE_GB], wide = (double)c->opt.v[OPT_MSM_WIDE_GB];
  size_t free_b = 0, total_b = 0;
  double free_gb = 1e9;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) free_gb = (double)free_b / 1e9;
  int first_choice = 0;  // what the policy picks when memory is no object
  for (int nw : {17, 18, 19, 20, 21, 22, 24, 26, 32}) {
    MsmGeom g = msm_geom_windows(nw);
    double gb = (double)n * (double)g.pt_entries * sizeof(Niels) / 1e9;
    if (nw == 17 && gb > wide) continue;
    if (gb > budget) continue;
    if (!first_choice) first_choice = nw;
    double reserve = gb >= 1.0 ? std::max(24.0, 5.0e-7 * (double)n * (double)n) : 0.25;  // room for the proof's working set next to a large table; a small table only has to fit
    if (gb + reserve <= free_gb || (nw == 32 && gb * 1.05 <= free_gb)) {
      if (nw > first_choice)
        fprintf(stderr, "spartan_hip: window tables of %zu generators cut from %d to %d windows (%.1f GB of device memory free): %d instead of %d additions per scalar\n",
                n, first_choice, nw, free_gb, nw, first_choice);
      *out = g;
      return true;
    }
  }
  return false;
}
const uint8_t* gens_compressed_bytes(const sp_gens* g, size_t* n) {
  const GensCacheEntry* e = (const GensCacheEntry*)g->cache_entry;
  *n = e->n;
  return e->mode == 0 ? e->in.data() : e->comp.data();  // the list is never modified while a handle on it exists
}
static int32_t gens_build(sp_ctx* c, const uint8_t* in, int mode, size_t n, uint8_t* comp_out, sp_gens** out) {
  if (!c || !in || !out || n == 0) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  size_t in_bytes = (mode == 0 ? 32 : 64) * n;
  std::lock_guard<std::mutex> lk(g_gens_mu);  // also serialises concurrent builds of the same table
  GensCacheEntry* hit = nullptr;
  for (auto& e : g_gens_cache)  // a resident table set serves every later handle on the same points, whatever width it was built with
    if (e.dev == c->dev && e.mode == mode && e.n == n && memcmp(e.in.data(), in, in_bytes) == 0) { hit = &e; break; }
  if (!hit) {
    MsmGeom geom;
    if (!choose_geom(c, n, &geom)) {
      fprintf(stderr, "spartan_hip: no window tables fit: %zu generators need at least %.2f GB of free device memory (32 windows)\n", n,
              (double)n * (double)msm_geom_windows(32).pt_entries * sizeof(Niels) / 1e9);
      return SP_ENOMEM;
    }
    const int wbits = geom.wbits;
    // scratch layout: [in bytes][pad][Pt n][comp 32n][bad int]
    size_t off_pts = (in_bytes + 255) & ~(size_t)255;
    size_t off_comp = off_pts + n * sizeof(Pt);
    size_t off_bad = off_comp + ((32 * n + 255) & ~(size_t)255);
    HIPCHK(hipStreamSynchronize(c->stream));
    SPCHK(ensure(&c->scratch, &c->scratch_cap, off_bad + 256));
    uint8_t* base = (uint8_t*)c->scratch;
    HIPCHK(hipMemcpyAsync(base, in, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(base + off_bad, 0, 4, c->stream));
    Niels* table = nullptr;
    HIPCHK(hipMalloc((void**)&table, n * geom.pt_entries * sizeof(Niels)));
    NielsP* table_lds = nullptr;
    int lds_bits = (int)c->opt.v[OPT_MSM_LDS_BITS];   // 0 or 6..10 (options.hip refuses the rest)  // 10 bits: 512 x 96 B = 48 KB per sub-table, double-buffered in 96 of a CU's 160 KB of LDS
    // THE DEFAULT PER GENERATOR SET (measured: profiles/r5_ab_msm_forms.txt). While the wide tables keep >= 12 bits (17-22 additions per scalar)
    // the gathered forms win at every size measured (2^20, 2^22, 2^24). When HBM is short and the policy above lands on 10 or 8 bits (26-32
    // additions, at 0.68 of the addition ceiling), the LDS-staged form does the same 26 additions at 0.83 from tables that are SMALLER (96-byte
    // packed entries instead of 128-byte lines): the set then gets the packed tables too and its row commits take that form unless msm.form says otherwise.
    bool prefer_lds = false;
    // (not when msm.wbits forces the width: a caller that asks for 8- or 10-bit gathered tables gets them, and nothing outside its budget: ADVICE r5)
    if (!lds_bits && geom.nwin >= 26 && n >= 512 && c->opt.v[OPT_MSM_WBITS] < 4 && c->opt.v[OPT_MSM_WINDOWS] < 17) { lds_bits = 10; prefer_lds = true; }
    if (lds_bits && hipMalloc((void**)&table_lds, n * msm_geom(lds_bits).pt_entries * sizeof(NielsP)) != hipSuccess) {
      (void)hipGetLastError();
      table_lds = nullptr;
      if (!prefer_lds) { (void)hipFree(table); return SP_ENOMEM; }   // asked for by option: an error; chosen by the policy: do without
      lds_bits = 0; prefer_lds = false;
    }
    if (prefer_lds) fprintf(stderr, "spartan_hip: %zu generators with %d-window gathered tables: row commitments of this set take the LDS-staged form (10-bit windows streamed through LDS: the same 26 additions at a higher rate)\n", n, geom.nwin);
    {
      ProfScope ps(c, PF_GENS_TABLE, (double)n * geom.pt_entries * sizeof(Niels));
      hipLaunchKernelGGL(k_points_load, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, base, mode, n, (Pt*)(base + off_pts),
                         mode == 1 ? base + off_comp : (uint8_t*)nullptr, (int*)(base + off_bad));
      size_t nt = n * (size_t)(geom.nwin + geom.nwide) * (size_t)(geom.tent < 128 ? 1 : geom.tent / 128);
      hipLaunchKernelGGL(k_table_build<Niels>, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, c->stream, (const Pt*)(base + off_pts), n, table, geom);
      if (lds_bits) {
        MsmGeom gl = msm_geom(lds_bits);
        size_t ntl = n * gl.nwin * (size_t)(gl.tent < 128 ? 1 : gl.tent / 128);
        hipLaunchKernelGGL(k_table_build<NielsP>, dim3((unsigned)((ntl + 63) / 64)), dim3(64), 0, c->stream, (const Pt*)(base + off_pts), n, table_lds, gl);
      }
    }
    int bad = 0;
    std::vector<uint8_t> comp(mode == 1 ? 32 * n : 0);
    int32_t rc = fetch_out(c, base + off_bad, &bad, 4);
    if (rc == SP_OK && mode == 1) rc = fetch_out(c, base + off_comp, comp.data(), 32 * n);
    if (rc == SP_OK && hipGetLastError() != hipSuccess) rc = SP_EHIP;
    if (rc != SP_OK || bad) {
      (void)hipFree(table);
      if (table_lds) (void)hipFree(table_lds);
      return rc != SP_OK ? rc : SP_EPOINT;
    }
    (void)wbits;
    g_gens_cache.push_back(GensCacheEntry{c->dev, mode, geom, n, 0, std::vector<uint8_t>(in, in + in_bytes), std::move(comp), table, table_lds, lds_bits, prefer_lds});
    hit = &g_gens_cache.back();
  }
  // a resident entry serves every later handle on the same points — but a context that asks for the LDS-staged form's tables must get them:
  // built for the cached entry now if it has none (msm.form = 1 silently took the gathered form otherwise); another width than
  // the one already there is reported and the resident tables kept
  if (const int want_lds = (int)c->opt.v[OPT_MSM_LDS_BITS]) {
    if (hit->table_lds && hit->wbits_lds != want_lds)
      fprintf(stderr, "spartan_hip: generator set of %zu points is resident with %d-bit LDS-form tables; msm.lds_bits = %d ignored for it\n", n, hit->wbits_lds, want_lds);
    if (!hit->table_lds) {
      MsmGeom gl = msm_geom(want_lds);
      NielsP* tl = nullptr;
      HIPCHK(hipStreamSynchronize(c->stream));
      size_t off_pts = (in_bytes + 255) & ~(size_t)255, off_bad = off_pts + n * sizeof(Pt) + ((32 * n + 255) & ~(size_t)255);
      SPCHK(ensure(&c->scratch, &c->scratch_cap, off_bad + 256));
      uint8_t* base = (uint8_t*)c->scratch;
      if (hipMalloc((void**)&tl, n * gl.pt_entries * sizeof(NielsP)) != hipSuccess) { (void)hipGetLastError(); return SP_ENOMEM; }
      HIPCHK(hipMemcpyAsync(base, hit->in.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemsetAsync(base + off_bad, 0, 4, c->stream));
      hipLaunchKernelGGL(k_points_load, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, base, mode, n, (Pt*)(base + off_pts), (uint8_t*)nullptr, (int*)(base + off_bad));
      size_t ntl = n * gl.nwin * (size_t)(gl.tent < 128 ? 1 : gl.tent / 128);
      hipLaunchKernelGGL(k_table_build<NielsP>, dim3((unsigned)((ntl + 63) / 64)), dim3(64), 0, c->stream, (const Pt*)(base + off_pts), n, tl, gl);
      if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) { (void)hipFree(tl); return SP_EHIP; }
      hit->table_lds = tl; hit->wbits_lds = want_lds;
    }
  }
  sp_gens* g = new (std::nothrow) sp_gens();
  if (!g) {
    if (hit->refs == 0) {  // just built for this call
      (void)hipFree(hit->table);
      if (hit->table_lds) (void)hipFree(hit->table_lds);
      g_gens_cache.pop_back();
    }
    return SP_ENOMEM;
  }
  hit->refs++;
  if (mode == 1 && comp_out) memcpy(comp_out, hit->comp.data(), 32 * n);
  g->ctx = c;
  g->n = n;
  g->table = hit->table;
  g->geom = hit->geom;
  g->derived = hit->mode == 1;
  g->prefer_lds = hit->prefer_lds;
  g->table_lds = hit->table_lds;
  g->geom_lds = msm_geom(hit->wbits_lds ? hit->wbits_lds : 10);
  g->cache_entry = hit;
  *out = g;
  return SP_OK;
}
extern "C" {
int32_t sp_gens_upload(sp_ctx* c, const uint8_t* compressed, size_t n, sp_gens** out) { return gens_build(c, compressed, 0, n, nullptr, out); }
int32_t sp_gens_from_uniform(sp_ctx* c, const uint8_t* uniform, size_t n, uint8_t* compressed_out, sp_gens** out) {
  return gens_build(c, uniform, 1, n, compressed_out, out);
}
size_t sp_gens_len(const sp_gens* g) { return g ? g->n : 0; }
size_t sp_gens_table_bytes(const sp_gens* g) {  // everything the set holds in HBM: the gathered tables and, when built, the packed LDS-form tables
  if (!g) return 0;
  return g->n * g->geom.pt_entries * sizeof(Niels) + (g->table_lds ? g->n * g->geom_lds.pt_entries * sizeof(NielsP) : 0);
}
void sp_gens_free(sp_gens* g) {
  if (!g) return;
  (void)hipSetDevice(g->ctx->dev);
  (void)hipStreamSynchronize(g->ctx->stream);
  (void)hipStreamSynchronize(g->ctx->stream_bg);  // a background commit may still be reading the tables
  {
    std::lock_guard<std::mutex> lk(g_gens_mu);
    GensCacheEntry* e = (GensCacheEntry*)g->cache_entry;
    if (--e->refs == 0) {
      host_commit_forget(e);
      (void)hipFree(e->table);
      if (e->table_lds) (void)hipFree(e->table_lds);
      for (auto it = g_gens_cache.begin(); it != g_gens_cache.end(); ++it)
        if (&*it == e) { g_gens_cache.erase(it); break; }
    }
  }
  delete g;
}
int sp_msm_window_bits(void) { return MSM_WBITS; }
int sp_gens_window_bits(const sp_gens* g) { return g ? g->geom.wbits : 0; }
int sp_gens_windows(const sp_gens* g) { return g ? g->geom.nwin : 0; }
// Window counts for TWO generator streams that one prover will hold side by side (SNARKGens: the gens_r1cs_sat stream, n_a points, commits
// w_a scalars per proof; the gens_r1cs_eval stream, n_b points, w_b scalars — 2^s and 6 * 2^s for SNARK::prove). choose_geom sees one set at
// a time: whichever is built first takes what it likes and the other what is left. Here the pair is chosen together: the (windows_a,
// windows_b) that minimises the mixed additions of a proof, w_a * windows_a + w_b * windows_b, among the pairs whose tables fit the free
// device memory less the proof's reserve (and msm.table_gb each); ties go to the smaller tables. 2^20: 17 / 17 (35.5 + 141.8 GB; one set
// at a time: 17 / 18); 2^22: 17 / 18 (the only pair that fits); 2^24: 22 / 20 (18.3 + 146 GB with 299 GB free; one at a time: 18 / 22, as much memory
// and 6 % more additions; 20 / 20 — 183 GB, fewer additions still — would leave the 2^24 proof too little). The caller sets option msm.windows to each result around the creation of its stream (0 = leave it to the per-set policy:
// returned when a geometry is forced by msm.wbits / msm.windows, or for streams too small to matter).
int32_t sp_gens_plan_pair(sp_ctx* c, size_t n_a, size_t n_b, double w_a, double w_b, int* windows_a, int* windows_b) {
  if (!c || !windows_a || !windows_b || n_a == 0 || n_b == 0) return SP_EINVAL;
  *windows_a = *windows_b = 0;
  if (c->opt.v[OPT_MSM_WBITS] >= 4 || c->opt.v[OPT_MSM_WINDOWS] >= 17 || c->opt.v[OPT_MSM_PLAN_PAIR] == 0) return SP_OK;
  HIPCHK(hipSetDevice(c->dev));
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return SP_OK; }
  const double budget = (double)c->opt.v[OPT_MSM_TABLE_GB];
  const size_t n_max = n_a > n_b ? n_a : n_b;
  auto gb = [](size_t n, int nw) { return (double)n * (double)msm_geom_windows(nw).pt_entries * sizeof(Niels) / 1e9; };
  if (gb(n_max, 17) < 1.0) return SP_OK;  // small sets: everything fits, the per-set policy gives 17 windows anyway
  const double avail = (double)free_b / 1e9 - std::max(24.0, 5.0e-7 * (double)n_max * (double)n_max);
  static const int kCand[] = {17, 18, 19, 20, 21, 22, 24, 26, 32};
  double best_cost = 1e300, best_gb = 1e300;
  for (int wa : kCand)
    for (int wb : kCand) {
      const double ga = gb(n_a, wa), gbb = gb(n_b, wb);
      if (ga > budget || gbb > budget || ga + gbb > avail) continue;
      const double cost = w_a * wa + w_b * wb;
      if (cost < best_cost - 1e-9 || (cost < best_cost + 1e-9 && ga + gbb < best_gb)) { best_cost = cost; best_gb = ga + gbb; *windows_a = wa; *windows_b = wb; }
    }
  return SP_OK;
}
}  // extern "C"
