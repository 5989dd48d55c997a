// spartan_amd: the context (streams, buffer pool, staging, completion flag) and its profiling records.
#include <sched.h>
#include <cctype>
#include "internal.hpp"

const char* kProfNames[PF_COUNT] = {"gens_table_build", "msm_rows_fixed", "msm_windows_fixed", "msm_reduce_pass", "msm_reduce_compress", "eq_expand", "sumcheck_eval",
                                    "table_bind", "sumcheck_bind_eval", "vecmat", "dot", "fq_reduce", "sparse", "ipa", "spark", "misc", "msm_var", "msm_points",
                                    "commit_rows_points"};

int32_t ensure(void** p, size_t* cap, size_t need) {
  if (*cap >= need) return SP_OK;
  if (*p) HIPCHK(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  size_t want = need + need / 4 + 4096;
  HIPCHK(hipMalloc(p, want));
  *cap = want;
  return SP_OK;
}
static size_t pool_class(size_t bytes) {
  size_t k = 4096;
  while (k < bytes) k <<= 1;
  return k;
}
int32_t pool_alloc(sp_ctx* c, size_t bytes, void** out) {
  size_t k = pool_class(bytes);
  auto it = c->pool.find(k);
  if (it != c->pool.end() && !it->second.empty()) {
    *out = it->second.back();
    it->second.pop_back();
    return SP_OK;
  }
  hipError_t e = hipMalloc(out, k);
  if (e != hipSuccess) {  // give cached buffers back to the driver and retry once
    (void)hipStreamSynchronize(c->stream);
    for (auto& kv : c->pool) { for (void* p : kv.second) (void)hipFree(p); kv.second.clear(); }
    e = hipMalloc(out, k);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP;
  }
  c->pool_bytes += k;
  return SP_OK;
}
void pool_release(sp_ctx* c, void* p, size_t bytes) {
  if (p) c->pool[pool_class(bytes)].push_back(p);
}
int32_t ensure_pinned(sp_ctx* c, size_t need) {
  if (c->pinned_cap >= need) return SP_OK;
  HIPCHK(hipStreamSynchronize(c->stream));  // an async copy may still read the old buffer
  if (c->pinned) HIPCHK(hipHostFree(c->pinned));
  c->pinned = nullptr;
  c->pinned_cap = 0;
  size_t want = need * 2 + 4096;
  HIPCHK(hipHostMalloc((void**)&c->pinned, want, hipHostMallocDefault));
  c->pinned_cap = want;
  return SP_OK;
}
// A staging pair of its own for calls that queue a host vector and return without waiting (sp_vecmat_dev): the buffers of
// stage_in are rewritten by the next call, which may come before this copy has run. The event guards the pair's own reuse.
int32_t vm_stage(sp_ctx* c, const void* src, size_t bytes, const void** dev) {
  if (c->vm_ev) HIPCHK(hipEventSynchronize(c->vm_ev));  // the previous copy out of vm_pinned (long done in practice)
  else HIPCHK(hipEventCreateWithFlags(&c->vm_ev, hipEventDisableTiming));
  if (c->vm_cap < bytes) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->vm_pinned) HIPCHK(hipHostFree(c->vm_pinned));
    if (c->vm_dstage) HIPCHK(hipFree(c->vm_dstage));
    c->vm_pinned = c->vm_dstage = nullptr;
    c->vm_cap = 0;
    size_t want = bytes * 2 + 4096;
    HIPCHK(hipHostMalloc((void**)&c->vm_pinned, want, hipHostMallocDefault));
    HIPCHK(hipMalloc((void**)&c->vm_dstage, want));
    c->vm_cap = want;
  }
  memcpy(c->vm_pinned, src, bytes);
  HIPCHK(hipMemcpyAsync(c->vm_dstage, c->vm_pinned, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->vm_ev, c->stream));
  *dev = c->vm_dstage;
  return SP_OK;
}
void prof_drain(sp_ctx* c) {
  if (c->pending.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->stream_bg);
  for (auto& r : c->pending) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    c->prof_ms[r.fam] += ms;
    c->prof_n[r.fam] += 1;
    if (r.shape) {
      ProfShape& ps = c->prof_shapes[std::make_pair(r.fam, r.shape)];
      ps.ms += ms; ps.n += 1; ps.bytes += r.bytes; ps.ops += r.ops;
      // where the launch lies on the context's clock (sp_prof_read_spans): launches of one family overlap — a background launch under a
      // foreground one, a launch queued while its predecessor still holds the CUs' LDS — so their durations do not add up to busy time
      float t0 = 0;
      if (c->prof_epoch && hipEventElapsedTime(&t0, c->prof_epoch, r.e0) == hipSuccess && c->prof_spans.size() < 65536)
      {
        unsigned long long tiles = 0;
        if (r.issued && hipMemcpy(&tiles, r.issued, 8, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); tiles = 0; }
        c->prof_spans.push_back(ProfSpan{r.fam, r.shape, (double)t0, (double)t0 + (double)ms, 64.0 * (double)tiles});
      }
      else (void)hipGetLastError();
    }
    else if (r.bytes >= 64e6) {  // the throughput-sized launches of the other families (>= 64 MB of algorithmic traffic) as one "shape" of their own:
      ProfShape& ps = c->prof_shapes[std::make_pair(r.fam, PROF_SHAPE_BIG)];  // bench.py reports them apart from the launch-sized ones
      ps.ms += ms; ps.n += 1; ps.bytes += r.bytes; ps.ops += r.ops;
    }
    c->free_events.push_back(r.e0);
    c->free_events.push_back(r.e1);
  }
  c->pending.clear();
}
// copy small host data to the device staging buffer at byte offset off
int32_t stage_in(sp_ctx* c, size_t off, const void* src, size_t bytes) {
  SPCHK(ensure_pinned(c, off + bytes));
  memcpy(c->pinned + off, src, bytes);
  HIPCHK(hipMemcpyAsync((uint8_t*)c->dstage + off, c->pinned + off, bytes, hipMemcpyHostToDevice, c->stream));
  return SP_OK;
}
void* stage_small(sp_ctx* c, size_t off, const void* src, size_t bytes) {
  memcpy(c->hmap + off, src, bytes);
  return c->hmap + off;
}
__global__ void k_done(volatile uint32_t* flag, uint32_t seq) { SP_FG_PRIO();
  __threadfence_system();
  *flag = seq;
}
// Wait until everything queued on the main stream has run. The stream is in-order, so the flag kernel runs after the
// kernels (and copies) before it have completed, and their results in host memory precede the flag on the way to the host.
uint32_t sync_post(sp_ctx* c) {
  uint32_t seq = ++c->done_seq;
  hipLaunchKernelGGL(k_done, dim3(1), dim3(1), 0, c->stream, c->done_flag, seq);
  return seq;
}
int32_t sync_wait(sp_ctx* c, uint32_t seq) {
  for (uint64_t spins = 1;; spins++) {
    if (*c->done_flag == seq) { c->sync_epoch++; return SP_OK; }
    if ((spins & 0xFFFFF) == 0) {  // every ~ms: a faulted queue never delivers the flag
      hipError_t e = hipStreamQuery(c->stream);
      if (e == hipSuccess) {
        if (*c->done_flag != seq) return SP_EHIP;
        c->sync_epoch++;
        return SP_OK;
      }
      if (e != hipErrorNotReady) {
        fprintf(stderr, "spartan_hip: stream failed: %s\n", hipGetErrorString(e));
        return SP_EHIP;
      }
    }
  }
}
int32_t sync_spin(sp_ctx* c) { return sync_wait(c, sync_post(c)); }
DoneSig sig_make(sp_ctx* c, size_t total_workgroups) {
  if (!c->done_counter) return sig_none();
  return DoneSig{c->done_flag, c->done_counter, ++c->done_seq, (uint32_t)total_workgroups, c->ktime};
}
// wait for a trip whose last kernel was launched with `sig` (falls back to the flag kernel when the signal is off)
int32_t sig_wait(sp_ctx* c, const DoneSig& sig) { return sig.flag ? sync_wait(c, sig.seq) : sync_spin(c); }
int32_t fetch_small(sp_ctx* c, void* hdst, size_t bytes) {
  SPCHK(sync_spin(c));
  memcpy(hdst, hres(c), bytes);
  return SP_OK;
}
int32_t ensure_dstage(sp_ctx* c, size_t need) {
  if (c->dstage_cap >= need) return SP_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  return ensure(&c->dstage, &c->dstage_cap, need);
}
// device -> host through pinned memory, synchronous
int32_t fetch_out(sp_ctx* c, const void* dsrc, void* hdst, size_t bytes) {
  SPCHK(ensure_pinned(c, bytes));
  HIPCHK(hipMemcpyAsync(c->pinned, dsrc, bytes, hipMemcpyDeviceToHost, c->stream));
  SPCHK(sync_spin(c));
  memcpy(hdst, c->pinned, bytes);
  return SP_OK;
}

extern "C" {

const char* sp_strerror(int32_t s) {
  switch (s) {
    case SP_OK: return "ok";
    case SP_EINVAL: return "invalid argument";
    case SP_ENOMEM: return "out of device memory";
    case SP_EHIP: return "HIP runtime error or no gfx950 device";
    case SP_EPOINT: return "invalid ristretto255 encoding";
    case SP_ESCALAR: return "not a canonical scalar (value >= q)";
    case SP_EINDEX: return "matrix entry outside the declared shape (row or column index too large)";
    default: return "unknown";
  }
}
const char* sp_version(void) { return "spartan_amd 0.1 (gfx950)"; }

static int32_t ctx_init(sp_ctx* c, int device_id);
int32_t sp_ctx_create(int device_id, sp_ctx** out) {
  if (!out) return SP_EINVAL;
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    fprintf(stderr, "spartan_hip: no HIP device available (this library has no CPU fallback)\n");
    return SP_EHIP;
  }
  if (device_id < 0 || device_id >= ndev) return SP_EINVAL;
  HIPCHK(hipSetDevice(device_id));
  sp_ctx* c = new (std::nothrow) sp_ctx();
  if (!c) return SP_ENOMEM;
  int32_t rc = ctx_init(c, device_id);
  if (rc != SP_OK) {  // release whatever was created before the failing step
    sp_ctx_destroy(c);
    return rc;
  }
  *out = c;
  return SP_OK;
}
// The proving thread and the device exchange ~330 small messages per proof over PCIe (launches, the completion flag, challenges): with the thread on
// the other socket every one of them crosses the inter-socket link as well — 22.2-22.8 ms per 2^20 proof from the GPU's own node against 22.7-23.4 from
// the other one or unpinned on one box of the pool, no difference on another (profiles/r6_ab_numa.txt): part of the "box-to-box" spread of the earlier rounds. Narrow the CALLING thread's affinity (threads it
// creates later inherit it; the pinned host pages allocated below are then first touched on that node) to the CPUs sysfs lists as local to the
// device's PCI function. Never widens a mask, does nothing when the lists do not intersect or sysfs has no answer.
static void pin_thread_to_device_node(int device_id) {
  char bus[32] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device_id) != hipSuccess) { (void)hipGetLastError(); return; }
  for (char* p = bus; *p; p++) *p = (char)tolower((unsigned char)*p);
  char path[128];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bus);
  FILE* f = fopen(path, "r");
  if (!f) return;
  char list[1024] = {0};
  const bool got = fgets(list, sizeof list, f) != nullptr;
  fclose(f);
  if (!got) return;
  cpu_set_t have, want;
  if (sched_getaffinity(0, sizeof have, &have) != 0) return;
  CPU_ZERO(&want);
  int n = 0;
  for (char* p = list; *p && *p != '\n';) {  // "64-127,192-255"
    char* end = nullptr;
    long lo = strtol(p, &end, 10), hi = lo;
    if (end == p) break;
    if (*end == '-') { p = end + 1; hi = strtol(p, &end, 10); if (end == p) break; }
    for (long k = lo; k <= hi && k < CPU_SETSIZE; k++)
      if (k >= 0 && CPU_ISSET((int)k, &have)) { CPU_SET((int)k, &want); n++; }
    p = *end == ',' ? end + 1 : end;
  }
  if (n >= 8 && n < CPU_COUNT(&have)) (void)sched_setaffinity(0, sizeof want, &want);  // a handful of CPUs would starve the threads this one creates (uploader, small-commitment worker)
}
static int32_t ctx_init(sp_ctx* c, int device_id) {
  c->dev = device_id;
  c->stream = c->stream_bg = c->stream_side = nullptr;
  c->sync_ev = c->side_ev = nullptr;
  c->scratch = c->scratch2 = c->dstage = nullptr;
  c->scratch_cap = c->scratch2_cap = c->dstage_cap = 0;
  c->pinned = nullptr;
  c->pinned_cap = 0;
  c->hmap = nullptr;
  c->done_flag = nullptr;
  c->sync_epoch = 0;
  c->eq_next = 0;
  for (int k = 0; k < 8; k++) c->eq_slot_epoch[k] = 0;
  c->opt = sp_default_options();
  if (c->opt.v[OPT_HOST_PIN_THREAD]) pin_thread_to_device_node(device_id);  // before the pinned host pages below are allocated
  c->device_encode = c->opt.v[OPT_ENCODE_DEVICE] != 0;  // diagnostic: keep every RFC 9496 encode on the GPU
  c->prof_on = 0;
  c->prof_mask = ~0ULL;
  c->pool_bytes = 0;
  memset(c->prof_ms, 0, sizeof c->prof_ms);
  memset(c->prof_n, 0, sizeof c->prof_n);
  memset(c->prof_bytes, 0, sizeof c->prof_bytes);
  memset(c->prof_ops, 0, sizeof c->prof_ops);
  {
    // main stream: the Fiat-Shamir critical path, highest priority; background stream: throughput MSMs queued under it,
    // lowest priority. (CU masks would be the cleaner partition, but hipExtStreamCreateWithCUMask is not honoured on this
    // platform: it succeeds, and a 1/8 mask runs an MSM exactly as fast as 8/8 — bench/bg_probe.py.)
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));
    HIPCHK(hipStreamCreateWithPriority(&c->stream_side, hipStreamNonBlocking, hi));
    HIPCHK(hipEventCreateWithFlags(&c->side_ev, hipEventDisableTiming));
    HIPCHK(hipStreamCreateWithPriority(&c->stream_bg, hipStreamNonBlocking, lo));
    HIPCHK(hipStreamCreateWithPriority(&c->stream_low, hipStreamNonBlocking, lo));
    // background MSMs: one 1024-thread workgroup per CU on half of the CUs (k_msm_rows_bg). Measured at 2^20 with the
    // derefs row half in the background, share in eighths 2 / 3 / 4 / 5 / 6 / 8 -> 63.1 / 59.2 / 58.0 / 59.0 / 61.5 / 62.5 ms
    // per proof (63.3 without the overlap): less and the MSM is not done when it is needed, more and the second
    // sum-check's kernels queue behind MSM workgroups. Round 3 (the foreground under the MSM got shorter: look-ahead, fused inner-product
    // rounds), share 3 / 4 / 5 / 6 -> 29.2 / 28.3 / 27.5 / 27.8 ms per proof (29.98 without the overlap): 5.
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    c->n_cus = prop.multiProcessorCount;
    c->bg_lds = 0;
    c->bg_blocks = c->n_cus * (int)c->opt.v[OPT_BG_EIGHTHS] / 8;
  }
  HIPCHK(hipHostMalloc((void**)&c->hmap, HMAP_SIZE, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&c->done_flag, 64, hipHostMallocDefault));
  *c->done_flag = 0;
  c->done_seq = 0;
  HIPCHK(hipMalloc((void**)&c->done_counter, 512));  // word 0: DoneSig::counter | words 4..: row tickets of the fused small commitment
  HIPCHK(hipMemset(c->done_counter, 0, 512));
  HIPCHK(hipMalloc((void**)&c->q_heads, 4 * (size_t)MSMQ_BLOCK_WORDS * MSMQ_BLOCKS));
#ifdef SP_KTIME
  if (c->opt.v[OPT_DEBUG_KTIME]) { HIPCHK(hipMalloc((void**)&c->ktime, 64 * 8)); HIPCHK(hipMemset(c->ktime, 0, 64 * 8)); }
#endif
  HIPCHK(hipEventCreateWithFlags(&c->sync_ev, hipEventDisableTiming));
  return SP_OK;
}
}  // extern "C"
// state derived from options (sp_ctx_set_option / sp_ctx_copy_options, options.hip); which < 0: all of it
void ctx_options_changed(sp_ctx* c, int which) {
  if (which < 0 || which == OPT_ENCODE_DEVICE) c->device_encode = c->opt.v[OPT_ENCODE_DEVICE] != 0;
  if (which < 0 || which == OPT_BG_EIGHTHS) c->bg_blocks = c->n_cus * (int)c->opt.v[OPT_BG_EIGHTHS] / 8;
#ifdef SP_KTIME
  if ((which < 0 || which == OPT_DEBUG_KTIME) && c->opt.v[OPT_DEBUG_KTIME] && !c->ktime && hipSetDevice(c->dev) == hipSuccess &&
      hipMalloc((void**)&c->ktime, 64 * 8) == hipSuccess)
    (void)hipMemset(c->ktime, 0, 64 * 8);
#endif
}
extern "C" {
void sp_ctx_destroy(sp_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->dev);
  (void)hipStreamSynchronize(c->stream);
  prof_drain(c);
  for (auto e : c->free_events) (void)hipEventDestroy(e);
  for (auto& kv : c->pool)
    for (void* p : kv.second) (void)hipFree(p);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->scratch2) (void)hipFree(c->scratch2);
  if (c->dstage) (void)hipFree(c->dstage);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->hmap) (void)hipHostFree(c->hmap);
  if (c->done_flag) (void)hipHostFree((void*)c->done_flag);
  if (c->done_counter) (void)hipFree(c->done_counter);
  if (c->prof_epoch) (void)hipEventDestroy(c->prof_epoch);
  if (c->q_heads) (void)hipFree(c->q_heads);
  if (c->ktime) (void)hipFree(c->ktime);
  if (c->vm_pinned) (void)hipHostFree(c->vm_pinned);
  if (c->vm_dstage) (void)hipFree(c->vm_dstage);
  if (c->vm_ev) (void)hipEventDestroy(c->vm_ev);
  if (c->em_pinned) (void)hipHostFree(c->em_pinned);
  if (c->em_ev) (void)hipEventDestroy(c->em_ev);
  if (c->sync_ev) (void)hipEventDestroy(c->sync_ev);
  if (c->side_ev) (void)hipEventDestroy(c->side_ev);
  if (c->stream_side) (void)hipStreamDestroy(c->stream_side);
  if (c->stream_bg) (void)hipStreamDestroy(c->stream_bg);
  if (c->stream_low) (void)hipStreamDestroy(c->stream_low);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}
#ifdef SP_KTIME
// diagnostic build only (not in the header): the in-kernel time stamps of the last instrumented launch, in 100 MHz ticks
int32_t sp_debug_ktime(sp_ctx* c, long long* out, int n) {
  if (!c || !c->ktime || n > 64) return SP_EINVAL;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, c->ktime, 8 * (size_t)n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(c->ktime, 0, 64 * 8));
  return SP_OK;
}
#endif
int sp_ctx_device(const sp_ctx* c) { return c ? c->dev : -1; }
uint64_t sp_ctx_trips(const sp_ctx* c) { return c ? c->sync_epoch : 0; }
int32_t sp_ctx_sync(sp_ctx* c) {
  if (!c) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  SPCHK(sync_spin(c));
  return hipGetLastError() == hipSuccess ? SP_OK : SP_EHIP;
}
int32_t sp_prof_enable(sp_ctx* c, int on) {
  if (!c) return SP_EINVAL;
  prof_drain(c);
  if (on && !c->prof_epoch) {  // the zero of the spans' clock: recorded once, on the main stream
    HIPCHK(hipSetDevice(c->dev));
    HIPCHK(hipEventCreate(&c->prof_epoch));
    HIPCHK(hipEventRecord(c->prof_epoch, c->stream));
    HIPCHK(hipEventSynchronize(c->prof_epoch));
  }
  c->prof_on = on;
  return SP_OK;
}
int32_t sp_prof_select(sp_ctx* c, const char* family) {
  if (!c) return SP_EINVAL;
  prof_drain(c);
  if (!family) { c->prof_mask = ~0ULL; return SP_OK; }
  for (int i = 0; i < PF_COUNT; i++)
    if (strcmp(kProfNames[i], family) == 0) { c->prof_mask = 1ULL << i; return SP_OK; }
  return SP_EINVAL;
}
int32_t sp_prof_reset(sp_ctx* c) {
  if (!c) return SP_EINVAL;
  prof_drain(c);
  memset(c->prof_ms, 0, sizeof c->prof_ms);
  memset(c->prof_n, 0, sizeof c->prof_n);
  memset(c->prof_bytes, 0, sizeof c->prof_bytes);
  memset(c->prof_ops, 0, sizeof c->prof_ops);
  c->prof_shapes.clear();
  c->prof_spans.clear();
  return SP_OK;
}
int32_t sp_prof_read_spans(sp_ctx* c, const char* family, uint64_t* shape, double* t0_ms, double* t1_ms, double* issued_adds, int cap) {
  if (!c || !family) return SP_EINVAL;
  prof_drain(c);
  int fam = -1;
  for (int i = 0; i < PF_COUNT; i++)
    if (strcmp(kProfNames[i], family) == 0) fam = i;
  if (fam < 0) return SP_EINVAL;
  int k = 0;
  for (auto& sp : c->prof_spans) {
    if (sp.fam != fam) continue;
    if (k < cap) {
      if (shape) shape[k] = sp.shape;
      if (t0_ms) t0_ms[k] = sp.t0;
      if (t1_ms) t1_ms[k] = sp.t1;
      if (issued_adds) issued_adds[k] = sp.issued;
    }
    k++;
  }
  return k;
}
int32_t sp_prof_read_ops(sp_ctx* c, double* alg_ops, int cap) {
  if (!c || !alg_ops) return SP_EINVAL;
  prof_drain(c);
  for (int i = 0; i < PF_COUNT && i < cap; i++) alg_ops[i] = c->prof_ops[i];
  return PF_COUNT;
}
int32_t sp_prof_read_shapes(sp_ctx* c, const char* family, uint64_t* shape, double* total_ms, uint64_t* launches, double* alg_bytes, double* alg_ops, int cap) {
  if (!c || !family) return SP_EINVAL;
  prof_drain(c);
  int fam = -1;
  for (int i = 0; i < PF_COUNT; i++)
    if (strcmp(kProfNames[i], family) == 0) fam = i;
  if (fam < 0) return SP_EINVAL;
  int k = 0;
  for (auto& kv : c->prof_shapes) {
    if (kv.first.first != fam) continue;
    if (k < cap) {
      if (shape) shape[k] = kv.first.second;
      if (total_ms) total_ms[k] = kv.second.ms;
      if (launches) launches[k] = kv.second.n;
      if (alg_bytes) alg_bytes[k] = kv.second.bytes;
      if (alg_ops) alg_ops[k] = kv.second.ops;
    }
    k++;
  }
  return k;
}
int32_t sp_prof_read(sp_ctx* c, const char** names, double* total_ms, uint64_t* launches, double* alg_bytes, int cap) {
  if (!c) return SP_EINVAL;
  prof_drain(c);
  for (int i = 0; i < PF_COUNT && i < cap; i++) {
    if (names) names[i] = kProfNames[i];
    if (total_ms) total_ms[i] = c->prof_ms[i];
    if (launches) launches[i] = c->prof_n[i];
    if (alg_bytes) alg_bytes[i] = c->prof_bytes[i];
  }
  return PF_COUNT;
}
}  // extern "C"
