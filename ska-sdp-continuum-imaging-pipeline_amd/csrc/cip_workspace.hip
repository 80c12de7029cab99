// cip_workspace.hip - per-thread state of the host API: the error string, the
// profiler, the (device, thread) workspace with its buffers, cached host
// tables, readback staging, FFT plans and side stream, and the call scope
// every entry point opens.
#include <cmath>
#include <mutex>
#include <thread>

#include "cip_host.h"

namespace cip {

static thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

void clear_error() { g_last_error.clear(); }

thread_local Profiler g_prof;

// Zero `bytes` at `p` on the workspace's side stream, ordered after the work
// already queued on s; join_side() makes s wait for it.
int zero_on_side(Workspace* ws, void* p, size_t bytes, hipStream_t s) {
  if (!ws->side) {
    CIP_HIP_CHECK(hipStreamCreateWithFlags(&ws->side, hipStreamNonBlocking));
    CIP_HIP_CHECK(hipEventCreateWithFlags(&ws->ev_fork, hipEventDisableTiming));
    CIP_HIP_CHECK(hipEventCreateWithFlags(&ws->ev_join, hipEventDisableTiming));
  }
  CIP_HIP_CHECK(hipEventRecord(ws->ev_fork, s));
  CIP_HIP_CHECK(hipStreamWaitEvent(ws->side, ws->ev_fork, 0));
  CIP_HIP_CHECK(hipMemsetAsync(p, 0, bytes, ws->side));
  CIP_HIP_CHECK(hipEventRecord(ws->ev_join, ws->side));
  return CIP_OK;
}

int join_side(Workspace* ws, hipStream_t s) {
  if (!ws->ev_join) return CIP_OK;  // no zero_on_side yet
  CIP_HIP_CHECK(hipStreamWaitEvent(s, ws->ev_join, 0));
  return CIP_OK;
}

int PlanScope::open(bool pipelined) {
  if (!pipelined) {
    // back to the parity-0 buffers: their last pipelined user may still be queued on s
    pl.parity = 0;
    return CIP_OK;
  }
  if (!pl.plan_stream) {
    // the plan streams at the lowest priority: the scatter on s keeps first
    // call on freed wave slots (C3 pipelined 21.58-21.62 vs 21.46-21.53
    // Gvis/s at the default priority, 21.15-21.24 at the highest,
    // profiles/r05v_ab_plan_priority.txt)
    int prio_lo = 0, prio_hi = 0;
    CIP_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    CIP_HIP_CHECK(hipStreamCreateWithPriority(&pl.plan_stream, hipStreamNonBlocking, prio_lo));
    CIP_HIP_CHECK(hipStreamCreateWithPriority(&pl.plan_stream1, hipStreamNonBlocking, prio_lo));
    CIP_HIP_CHECK(hipEventCreateWithFlags(&pl.ev_planned, hipEventDisableTiming));
    CIP_HIP_CHECK(hipEventCreateWithFlags(&pl.ev_entry, hipEventDisableTiming));
    for (hipEvent_t& e : pl.ev_done) {
      CIP_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      // the first pipelined calls: the planner starts after the work already on s
      CIP_HIP_CHECK(hipEventRecord(e, s));
    }
  }
  if (pl.plan_unscoped) {
    // a planner ran on s since the last pipelined call: its buffers (parity
    // 0) may still be read there - both plan streams wait for it
    CIP_HIP_CHECK(hipEventRecord(pl.ev_entry, s));
    CIP_HIP_CHECK(hipStreamWaitEvent(pl.plan_stream, pl.ev_entry, 0));
    CIP_HIP_CHECK(hipStreamWaitEvent(pl.plan_stream1, pl.ev_entry, 0));
    pl.plan_unscoped = false;
  }
  // this parity's planner buffers: after their last user, the call before the
  // previous one. Not after s: the caller promised the inputs are complete
  pl.parity ^= 1;
  ps = pl.parity ? pl.plan_stream1 : pl.plan_stream;
  CIP_HIP_CHECK(hipStreamWaitEvent(ps, pl.ev_done[pl.parity], 0));
  pl.parity_scope = armed = true;
  joined = false;
  return CIP_OK;
}

int PlanScope::join() {
  if (joined) return CIP_OK;
  joined = true;
  pl.parity_scope = false;
  CIP_HIP_CHECK(hipEventRecord(pl.ev_planned, ps));
  CIP_HIP_CHECK(hipStreamWaitEvent(s, pl.ev_planned, 0));
  return CIP_OK;
}

PlanScope::~PlanScope() {
  (void)join();
  if (armed) (void)hipEventRecord(pl.ev_done[pl.parity], s);
}

void PlanPipeline::destroy() {
  for (hipStream_t st : {plan_stream, plan_stream1})
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  for (hipEvent_t e : {ev_done[0], ev_done[1], ev_planned, ev_entry})
    if (e) (void)hipEventDestroy(e);
  *this = PlanPipeline();
}

static std::mutex g_ws_mutex;
// One workspace per (device, host thread): calls from different threads (e.g.
// two inverts in flight on one GPU, each thread on its own stream) never
// share buffers, the side stream or the clean-grid state. A workspace holds
// the uv grid (16 nu nv bytes) and planner buffers that grow with the
// visibility count, so it lives only as long as its thread: a thread-exit hook
// frees the workspaces of every worker thread that made one (dask worker
// pools keep HBM use at one workspace per live thread), and
// cip_release_workspace frees the calling thread's on demand.
static std::map<std::pair<int, std::thread::id>, Workspace*> g_ws;
// the thread that loaded the library: its workspaces are left to process
// teardown (its thread-exit hook runs inside exit(), where the HIP runtime
// may already be shutting down)
static const std::thread::id g_load_thread = std::this_thread::get_id();

static void destroy_workspace(Workspace* ws) {
  // the workspace's device current while its buffers go (the reaper may run on
  // a thread whose current device differs), and a CIP_ASYNC call's work drained
  // first: its scatter / FFT may still be queued on the caller's stream
  int prev_dev = -1;
  (void)hipGetDevice(&prev_dev);
  if (prev_dev != ws->device) (void)hipSetDevice(ws->device);
  if (ws->async_queued) (void)hipStreamSynchronize(ws->async_stream);
  ws->pipeline.destroy();
  for (auto& kv : ws->bufs)
    if (kv.second.ptr) (void)hipFree(kv.second.ptr);
  for (auto& p : ws->plans) (void)hipfftDestroy(p.h);
  if (ws->pinned) (void)hipHostFree(ws->pinned);
  for (auto& kv : ws->tables) {
    if (kv.second.staging) (void)hipHostFree(kv.second.staging);
    if (kv.second.uploaded) (void)hipEventDestroy(kv.second.uploaded);
  }
  if (ws->side) {
    (void)hipStreamSynchronize(ws->side);
    (void)hipStreamDestroy(ws->side);
  }
  if (ws->ev_fork) (void)hipEventDestroy(ws->ev_fork);
  if (ws->ev_join) (void)hipEventDestroy(ws->ev_join);
  const int dev = ws->device;
  delete ws;
  if (prev_dev >= 0 && prev_dev != dev) (void)hipSetDevice(prev_dev);
}

// Frees the calling thread's workspaces (every device) when the thread ends.
struct WorkspaceReaper {
  bool armed = false;
  ~WorkspaceReaper() {
    if (!armed || std::this_thread::get_id() == g_load_thread) return;
    std::vector<Workspace*> mine;
    {
      std::lock_guard<std::mutex> lock(g_ws_mutex);
      for (auto it = g_ws.begin(); it != g_ws.end();) {
        if (it->first.second == std::this_thread::get_id()) {
          mine.push_back(it->second);
          it = g_ws.erase(it);
        } else {
          ++it;
        }
      }
    }
    for (Workspace* ws : mine) destroy_workspace(ws);
  }
};
static thread_local WorkspaceReaper g_reaper;

static Workspace* workspace() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  const auto key = std::make_pair(dev, std::this_thread::get_id());
  g_reaper.armed = true;
  std::lock_guard<std::mutex> lock(g_ws_mutex);
  auto it = g_ws.find(key);
  if (it != g_ws.end()) return it->second;
  Workspace* ws = new Workspace();
  ws->device = dev;
  g_ws[key] = ws;
  return ws;
}

static void* buf_named(Workspace* ws, const std::string& name, size_t bytes) {
  DevBuf& b = ws->bufs[name];
  if (b.bytes < bytes) {
    if (b.ptr) ws->saved_valid = false;  // the saved plan may point into it
    if (b.ptr) (void)hipFree(b.ptr);
    b.ptr = nullptr;
    b.bytes = 0;
    // 12.5 % headroom so slowly growing inputs do not reallocate every call
    const size_t want = bytes + bytes / 8;
    if (hipMalloc(&b.ptr, want) != hipSuccess) {
      (void)hipGetLastError();
      set_error(CIP_ENOMEM, "hipMalloc failed for workspace buffer " + name);
      return nullptr;
    }
    b.bytes = want;
  }
  return b.ptr;
}

void* buf_bytes(Workspace* ws, const char* name, size_t bytes) {
  return buf_named(ws, ws->pipeline.odd_names() ? std::string(name) + "~1" : std::string(name), bytes);
}

double* grid_buffer(Workspace* ws, size_t bytes) {
  if (ws->bufs["grid"].bytes < bytes) ws->grid_zero.invalidate();  // buf_named reallocates: not known zero
  return (double*)buf_named(ws, "grid", bytes);
}

// grow-only pinned host memory (the readback staging and each table's own)
static void* pinned_grow(void** p, size_t* have, size_t bytes) {
  if (*have < bytes) {
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *have = 0;
    if (hipHostMalloc(p, bytes) != hipSuccess) {
      *p = nullptr;
      set_error(CIP_ENOMEM, "hipHostMalloc failed");
      return nullptr;
    }
    *have = bytes;
  }
  return *p;
}

void* pinned(Workspace* ws, size_t bytes) { return pinned_grow(&ws->pinned, &ws->pinned_bytes, bytes); }

int readback_bytes(Workspace* ws, hipStream_t s, std::initializer_list<DevSrc> src, void** host) {
  const auto slot = [](size_t bytes) { return (bytes + 7) & ~(size_t)7; };
  size_t total = 0;
  for (const DevSrc& c : src) total += slot(c.bytes);
  char* h = (char*)pinned(ws, total);
  if (!h) return CIP_ENOMEM;
  size_t at = 0;
  for (const DevSrc& c : src) {
    if (c.dev) CIP_HIP_CHECK(hipMemcpyAsync(h + at, c.dev, c.bytes, hipMemcpyDeviceToHost, s));
    at += slot(c.bytes);
  }
  CIP_HIP_CHECK(hipStreamSynchronize(s));
  *host = h;
  return CIP_OK;
}

int host_table_open(Workspace* ws, const char* name, const std::vector<double>& key, size_t bytes, void** staging) {
  HostTable& t = ws->tables[name];
  *staging = nullptr;
  if (t.key == key) return CIP_OK;
  t.key.clear();
  if (!t.uploaded) {
    CIP_HIP_CHECK(hipEventCreateWithFlags(&t.uploaded, hipEventDisableTiming));
  } else {
    // the last upload has read the staging (it has, unless that stream is far behind)
    CIP_HIP_CHECK(hipEventSynchronize(t.uploaded));
  }
  if (!pinned_grow(&t.staging, &t.staging_bytes, bytes)) return CIP_ENOMEM;
  *staging = t.staging;
  return CIP_OK;
}

int host_table_upload(Workspace* ws, const char* name, const std::vector<double>& key, void* dev, size_t bytes,
                      hipStream_t s) {
  HostTable& t = ws->tables[name];
  CIP_HIP_CHECK(hipMemcpyAsync(dev, t.staging, bytes, hipMemcpyHostToDevice, s));
  CIP_HIP_CHECK(hipEventRecord(t.uploaded, s));
  t.key = key;
  return CIP_OK;
}

int fft_plan(Workspace* ws, int64_t nu, int64_t nv, hipStream_t s, hipfftHandle* out) {
  for (auto& p : ws->plans)
    if (p.nu == nu && p.nv == nv) {
      if (hipfftSetStream(p.h, s) != HIPFFT_SUCCESS) return set_error(CIP_EHIP, "hipfftSetStream failed");
      *out = p.h;
      return CIP_OK;
    }
  hipfftHandle h;
  if (hipfftPlan2d(&h, (int)nu, (int)nv, HIPFFT_Z2Z) != HIPFFT_SUCCESS)
    return set_error(CIP_EHIP, "hipfftPlan2d failed");
  if (hipfftSetStream(h, s) != HIPFFT_SUCCESS) return set_error(CIP_EHIP, "hipfftSetStream failed");
  ws->plans.push_back({h, nu, nv});
  *out = h;
  return CIP_OK;
}

// exp(+2 pi i m / n), m < n, for the pruned FFT passes (cached per length)
int fft_twiddles(Workspace* ws, int64_t n, hipStream_t s, double** out) {
  const std::string name = "fft_twiddle_" + std::to_string(n);
  double* tw = buf<double>(ws, name.c_str(), 2 * n);
  if (!tw) return CIP_ENOMEM;
  *out = tw;
  return host_table(ws, name.c_str(), {(double)n}, tw, sizeof(double) * 2 * n, s, [n](void* staging) {
    double* h = (double*)staging;
    for (int64_t m = 0; m < n; ++m) {
      // long double arguments: each entry correctly rounded (to within an ulp)
      const long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)n;
      h[2 * m] = (double)cosl(a);
      h[2 * m + 1] = (double)sinl(a);
    }
  });
}

int begin_call(void* hip_stream, bool profiled, Call* c) {
  g_last_error.clear();
  c->s = (hipStream_t)hip_stream;
  Workspace* ws = workspace();
  if (!ws) return set_error(CIP_EHIP, "no HIP device");
  // an earlier call's work queued on another stream (NULL is a stream too: the default one)
  if (ws->async_queued && ws->async_stream != c->s) CIP_HIP_CHECK(hipStreamSynchronize(ws->async_stream));
  ws->async_queued = false;
  c->ws = ws;  // from here ~Call notes the stream
  c->profiled = profiled;
  if (profiled) {
    g_prof.reset();
    c->t0 = g_prof.mark(c->s);
  }
  return CIP_OK;
}

int end_call(Call& c, bool wait) {
  if (c.profiled) g_prof.span(5, c.t0, g_prof.mark(c.s));
  if (!wait && !(c.profiled && g_prof.on)) return CIP_OK;  // queued: ~Call notes the stream
  CIP_HIP_CHECK(hipStreamSynchronize(c.s));
  c.synced = true;
  if (c.profiled) g_prof.finish();
  return CIP_OK;
}

Call::~Call() {
  if (ws && !synced) ws->async_queued = true, ws->async_stream = s;
}

}  // namespace cip

using namespace cip;

extern "C" {

const char* cip_last_error(void) { return g_last_error.c_str(); }

const char* cip_build_info(void) { return "libcip_hip gfx950 (CDNA4) v0.1.0"; }

int cip_profile_enable(int on) {
  g_prof.on = (on != 0);
  return CIP_OK;
}

int cip_profile_last(double* ms, int64_t* counts) {
  if (ms)
    for (int i = 0; i < CIP_PROFILE_PHASES; ++i) ms[i] = g_prof.ms[i];
  if (counts)
    for (int i = 0; i < CIP_PROFILE_COUNTS; ++i) counts[i] = g_prof.counts[i];
  return CIP_OK;
}

int cip_release_workspace(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return set_error(CIP_EHIP, "no HIP device");
  std::lock_guard<std::mutex> lock(g_ws_mutex);
  auto it = g_ws.find(std::make_pair(dev, std::this_thread::get_id()));
  if (it == g_ws.end()) return CIP_OK;
  Workspace* ws = it->second;
  g_ws.erase(it);
  destroy_workspace(ws);
  return CIP_OK;
}

}  // extern "C"
